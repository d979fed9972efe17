"""grx_fetch_post_step (the fused launch behind a Fetch step) against the launches it replaces: grx_order_by_cost_slots followed by grx_fetch_commit_rows, on cloned
buffers.  Every output is compared bit for bit: `order`, `ema`, every committed row, `final_packed`, `status`, and the compact block of terminal rows against a gather of
the unfused path's `final_packed`.  The sort keys are unique (cost, world) pairs, so there is one right permutation and no tolerance."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NQ, NV, MOCAP, OD = 15, 14, 7, 25
PW = OD + 8
ALPHA = 0.1


def _buffers(n, seed):
    """live + staged world rows of a Fetch batch, filled with noise (the commit copies words, it computes nothing)"""
    import torch

    g = torch.Generator(device="cuda:0"); g.manual_seed(seed)
    r = lambda *s: torch.randn(*s, device="cuda:0", generator=g)
    live = dict(qpos=r(n, NQ), qvel=r(n, NV), qacc_ws=r(n, NV), mocap=r(n, MOCAP), aux=r(n, 8), goal=r(n, 3), obs=r(n, OD), achieved=r(n, 3), packed=r(n, PW),
                final_packed=r(n, PW), status=torch.randint(0, 1 << 20, (n,), device="cuda:0", dtype=torch.int32, generator=g))
    staged = dict(qpos=r(n, NQ), qvel=r(n, NV), qacc_ws=r(n, NV), mocap=r(n, MOCAP), aux=r(n, 8), goal=r(n, 3), obs=r(n, OD), achieved=r(n, 3),
                  status=torch.randint(0, 16, (n,), device="cuda:0", dtype=torch.int32, generator=g))
    return live, staged


def _commit_args(idx, k, live, staged):
    from gymnasium_robotics_amd import _native

    return _native.FetchCommitArgsStruct(idx.data_ptr(), k, NQ, NV, MOCAP, OD,
                                         *[staged[f].data_ptr() for f in ("qpos", "qvel", "qacc_ws", "mocap", "aux", "goal", "obs", "achieved", "status")],
                                         *[live[f].data_ptr() for f in ("qpos", "qvel", "qacc_ws", "mocap", "aux", "goal", "obs", "achieved", "packed", "final_packed", "status")])


def _costs(n, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "equal":
        return np.full(n, 1234, np.int32)
    c = rng.integers(900, 1500, n).astype(np.int32)      # many ties: the world index decides
    if kind == "tail":      # a handful of worlds above twice the cheapest of their slice (the tail-aware placement of the two-worlds-per-slot regime)
        c[rng.choice(n, 24, replace=False)] = rng.integers(2000, 9000, 24)
    return c


def _run(n, slots, cost_kind, k, use_ema=True, use_order=True, seed=0):
    import torch

    from gymnasium_robotics_amd import _native

    L = _native.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(seed + 7)
    cost = torch.from_numpy(_costs(n, cost_kind, seed)).cuda()
    ema0 = torch.from_numpy(rng.uniform(800, 1600, n).astype(np.float32)).cuda()
    idx = torch.from_numpy(rng.permutation(n)[:max(k, 1)].astype(np.int32)).cuda()
    live, staged = _buffers(n, seed)
    clone = lambda d: {f: t.clone() for f, t in d.items()}

    # the launches it replaces
    ref, ema_ref, order_ref = clone(live), ema0.clone(), torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    if use_order:
        _native.check(L.grx_order_by_cost_slots(cost.data_ptr(), ema_ref.data_ptr() if use_ema else None, ALPHA, n, slots, order_ref.data_ptr(), stream))
    _native.check(L.grx_fetch_commit_rows(ctypes.byref(_commit_args(idx, k, ref, staged)), stream))
    rows_ref = ref["final_packed"][idx[:k].long()]

    # the fused launch
    new, ema_new, order_new = clone(live), ema0.clone(), torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    rows_new = torch.full((max(k, 1), PW), float("nan"), device="cuda:0")
    _native.check(L.grx_fetch_post_step(cost.data_ptr() if use_order else None, ema_new.data_ptr() if (use_ema and use_order) else None, ALPHA, n, slots,
                                        order_new.data_ptr() if use_order else None, ctypes.byref(_commit_args(idx, k, new, staged)), rows_new.data_ptr(), stream))
    torch.cuda.synchronize()

    assert torch.equal(order_new, order_ref)
    if use_order:
        assert sorted(order_new.cpu().tolist()) == list(range(n))
    assert torch.equal(ema_new.view(torch.int32), ema_ref.view(torch.int32))
    assert use_ema and use_order or torch.equal(ema_new, ema0)
    for f in live:
        a, b = new[f], ref[f]
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), f
    assert torch.equal(rows_new[:k].view(torch.int32), rows_ref.view(torch.int32))
    if k:      # something was committed at all: the listed worlds' rows changed
        assert not torch.equal(new["qpos"], live["qpos"])
    else:
        assert all(torch.equal(new[f], live[f]) for f in ("qpos", "packed", "status", "final_packed"))


@pytest.mark.parametrize("n, slots, cost_kind", [(64, 0, "random"), (1048, 0, "random"), (4096, 256, "tail"), (4096, 256, "equal"), (1048, 100, "equal")])
def test_post_step_is_order_then_commit(n, slots, cost_kind):
    _run(n, slots, cost_kind, k=min(n, 83))


@pytest.mark.parametrize("k", [0, 1, 1048])
def test_post_step_list_lengths(k):
    _run(1048, 0, "random", k=k, seed=k + 1)


def test_post_step_without_ema():
    _run(4096, 256, "tail", k=82, use_ema=False)


def test_post_step_without_order():
    _run(1048, 0, "random", k=82, use_order=False)


def test_post_step_order_alone_and_nothing():
    """commit NULL: the ordering half alone; neither half: no launch, no error.  A slice of more than 256 worlds per thread pair (16 384 worlds: 8 keys per thread)."""
    import torch

    from gymnasium_robotics_amd import _native

    L = _native.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for n, slots in ((8192, 256), (16384, 256)):
        cost = torch.from_numpy(_costs(n, "tail", n)).cuda()
        ema = torch.full((n,), 1000.0, device="cuda:0")
        e1, e2 = ema.clone(), ema.clone()
        o1, o2 = torch.zeros(n, dtype=torch.int32, device="cuda:0"), torch.zeros(n, dtype=torch.int32, device="cuda:0")
        _native.check(L.grx_order_by_cost_slots(cost.data_ptr(), e1.data_ptr(), ALPHA, n, slots, o1.data_ptr(), stream))
        _native.check(L.grx_fetch_post_step(cost.data_ptr(), e2.data_ptr(), ALPHA, n, slots, o2.data_ptr(), None, None, stream))
        torch.cuda.synchronize()
        assert torch.equal(o1, o2) and torch.equal(e1.view(torch.int32), e2.view(torch.int32))
    _native.check(L.grx_fetch_post_step(None, None, ALPHA, 1048, 0, None, None, None, stream))
    assert L.grx_fetch_post_step(None, None, ALPHA, 1048, 0, o1.data_ptr(), None, None, stream) != 0      # order without cost
