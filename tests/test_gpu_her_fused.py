"""The fused HER launches against the launch sequences they replace, bit for bit:

1. grx_her_append (both row copies + the episode marks of the reset worlds, from an index list or from a mask) against two copies + grx_her_mark_resets;
2. grx_her_draw_relabel / grx_her_sample_relabel (draws and rows in one kernel) against grx_her_sample_final + grx_her_relabel;
3. a FetchPickAndPlace rollout with HerReplay on the fused tail (grx_fetch_post_step, grx_her_append, grx_her_draw_relabel) against the same rollout with
   GRX_FETCH_FUSED_TAIL=0.

On `order` in part 3: a world's cost is the wall-clock duration the step kernel measured for it, so two environments never see the same costs and their orders differ
however they are computed (results do not depend on the order).  The fused environment's order is therefore checked after every step against grx_order_by_cost_slots
run on ITS costs and ITS moving average of the step before -- the launch the fused one replaces, on the same inputs."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _stream():
    import torch

    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(x):
    import torch

    return x.view(torch.int32) if x.dtype == torch.float32 else x


# ------------------------------------------------------------------------------------------------ 1. append
@pytest.mark.parametrize("source", ["list", "mask"])
@pytest.mark.parametrize("track", [True, False])
def test_append_kernel_is_copies_and_marks(source, track):
    import torch

    from gymnasium_robotics_amd import _native

    L = _native.lib()
    N, T, W, A = 8, 5, 33, 4
    R = T + 1
    resets = [[], [3], list(range(N)), [5], [5], [], [0, 7], [2], list(range(N)), list(range(N)), [1, 2, 3], [], [6]]      # 13 appends: the ring of 6 rows wraps twice
    assert len(resets) == 13
    g = torch.Generator(device="cuda:0"); g.manual_seed(3)
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device="cuda:0")
    mk = lambda: dict(episode=z(R, N, W), actions=z(R, N, A), start=z(N, dtype=torch.int32), prev=z(N, dtype=torch.int32), term=torch.full((N,), -1, dtype=torch.int32, device="cuda:0"))
    ref, new = mk(), mk()
    for step, lst in enumerate(resets):
        t, r = step + 1, (step + 1) % R
        packed, act = torch.randn(N, W, device="cuda:0", generator=g), torch.randn(N, A, device="cuda:0", generator=g)
        mask = torch.zeros(N, dtype=torch.bool, device="cuda:0")
        if lst:
            mask[torch.tensor(lst, device="cuda:0")] = True
        idx = torch.tensor(lst + [N + 5, -1], dtype=torch.int32, device="cuda:0")      # (entries past `count` are never read)
        # the copy-and-mark path
        ref["actions"][r].copy_(act); ref["episode"][r].copy_(packed)
        _native.check(L.grx_her_mark_resets(mask.data_ptr(), N, t, ref["start"].data_ptr(), ref["prev"].data_ptr() if track else None, ref["term"].data_ptr() if track else None, _stream()))
        # one kernel
        a = _native.HerAppendArgsStruct()
        a.packed, a.action, a.row_dst, a.act_dst = packed.data_ptr(), act.data_ptr(), new["episode"][r].data_ptr(), new["actions"][r].data_ptr()
        a.n_row, a.n_act, a.n_worlds, a.t, a.W = N * W, N * A, N, t, W
        a.start = new["start"].data_ptr()
        if track:
            a.prev_start, a.term_t = new["prev"].data_ptr(), new["term"].data_ptr()
        if source == "list":
            a.list, a.count = idx.data_ptr(), len(lst)
        else:
            a.mask = mask.data_ptr()
        _native.check(L.grx_her_append(ctypes.byref(a), _stream()))
        torch.cuda.synchronize()
        for f in ref:
            assert torch.equal(_bits(new[f]), _bits(ref[f])), (step, f)
    assert int(ref["start"].min()) >= 9 and (not track or int(ref["term"].max()) == 13)


def test_append_from_a_device_count_and_argument_checks():
    import torch

    from gymnasium_robotics_amd import _native

    L = _native.lib()
    N, W, A = 8, 33, 4
    packed, act = torch.randn(N, W, device="cuda:0"), torch.randn(N, A, device="cuda:0")
    row, arow, start = torch.zeros(N, W, device="cuda:0"), torch.zeros(N, A, device="cuda:0"), torch.zeros(N, dtype=torch.int32, device="cuda:0")
    idx, cnt = torch.tensor([4, 1, 6, 0], dtype=torch.int32, device="cuda:0"), torch.tensor([2], dtype=torch.int32, device="cuda:0")
    a = _native.HerAppendArgsStruct()
    a.packed, a.action, a.row_dst, a.act_dst, a.start = packed.data_ptr(), act.data_ptr(), row.data_ptr(), arow.data_ptr(), start.data_ptr()
    a.n_row, a.n_act, a.n_worlds, a.t, a.W = N * W, N * A, N, 7, W
    a.list, a.count_dev, a.count = idx.data_ptr(), cnt.data_ptr(), 4      # the device word wins
    _native.check(L.grx_her_append(ctypes.byref(a), _stream()))
    torch.cuda.synchronize()
    assert torch.equal(row, packed) and torch.equal(arow, act) and start.cpu().tolist() == [0, 7, 0, 0, 7, 0, 0, 0]
    a.mask = idx.data_ptr()
    assert L.grx_her_append(ctypes.byref(a), _stream()) != 0 and b"list or as a mask" in L.grx_last_error()
    a.mask, a.term_t = None, start.data_ptr()
    assert L.grx_her_append(ctypes.byref(a), _stream()) != 0 and b"go together" in L.grx_last_error()


# ------------------------------------------------------------------------------------------------ 2. draws + rows in one kernel
KINDS = [(0, 3, 0.05), (1, 15, 0.01), (2, 2, 0.45), (3, 7, 0.01)]      # reward kind, goal_dim, threshold
N_W, T_H, OD, AD = 64, 10, 11, 5


def _ring(kind, gd, terminal, all_reset, seed):
    import torch

    from gymnasium_robotics_amd import _native

    g = torch.Generator(device="cuda:0"); g.manual_seed(seed)
    W, R, t_now = OD + 2 * gd + 2, T_H + 1, 23      # the ring has wrapped twice
    rows, acts = torch.randn(R, N_W, W, device="cuda:0", generator=g) * 0.05, torch.randn(R, N_W, AD, device="cuda:0", generator=g)
    rng = np.random.default_rng(seed)
    start = rng.integers(t_now - 14, t_now, N_W).astype(np.int32)      # some episodes began before the oldest row still in the ring
    prev, term = np.zeros(N_W, np.int32), np.full(N_W, -1, np.int32)
    just = np.ones(N_W, bool) if all_reset else (rng.random(N_W) < 0.3)      # worlds reset in this very step
    prev[just], term[just], start[just] = start[just] - 3, t_now, t_now
    old = ~just & (rng.random(N_W) < 0.3)      # an earlier episode end whose mark is still around
    term[old], prev[old] = start[old], start[old] - 20
    dev = lambda x: torch.from_numpy(x).cuda()
    st = dict(rows=rows, acts=acts, start=dev(start), prev=dev(prev), term=dev(term), term_rows=torch.randn(N_W, W, device="cuda:0", generator=g) * 0.05, t_now=t_now, W=W)

    def args(out, idx=None):
        a = _native.HerArgsStruct()
        a.rows, a.acts, a.out = rows.data_ptr(), acts.data_ptr(), out.data_ptr()
        a.T, a.N, a.W, a.obs_dim, a.goal_dim, a.act_dim = T_H, N_W, W, OD, gd, AD
        a.kind, a.p0, a.p1, a.sparse, a.ignore_z = kind, KINDS[kind][2], 0.1, seed & 1, int(kind == 3)
        if terminal:
            a.term_rows, a.term_t = st["term_rows"].data_ptr(), st["term"].data_ptr()
        if idx is not None:
            a.t_idx, a.w_idx, a.t_goal = (x.data_ptr() for x in idx)
        return a

    return st, args


@pytest.mark.parametrize("terminal", [True, False])
@pytest.mark.parametrize("kind, gd, thr", KINDS)
def test_draw_relabel_is_sample_then_relabel(kind, gd, thr, terminal):
    import torch

    from gymnasium_robotics_amd import _native

    L = _native.lib()
    st, args = _ring(kind, gd, terminal, False, seed=kind * 2 + int(terminal))
    OW = 2 * OD + 3 * gd + AD + 2
    prev = st["prev"].data_ptr() if terminal else None
    for call, B in enumerate((1, 255, 257, 4 * N_W)):
        idx = [torch.empty(B, dtype=torch.int32, device="cuda:0") for _ in range(3)]
        ref, new, new_v = (torch.full((B, OW), float("nan"), device="cuda:0") for _ in range(3))
        _native.check(L.grx_her_sample_final(st["start"].data_ptr(), prev, st["term"].data_ptr() if terminal else None, N_W, st["t_now"], T_H, 4, 11, call, B,
                                             *[x.data_ptr() for x in idx], _stream()))
        _native.check(L.grx_her_relabel(ctypes.byref(args(ref, idx)), B, _stream()))
        _native.check(L.grx_her_draw_relabel(ctypes.byref(args(new)), st["start"].data_ptr(), prev, st["t_now"], 4, 11, call, B, None, _stream()))
        scratch, valid = torch.zeros(3 * B, dtype=torch.int32, device="cuda:0"), torch.full((1,), -7, dtype=torch.int32, device="cuda:0")
        _native.check(L.grx_her_sample_relabel(ctypes.byref(args(new_v)), st["start"].data_ptr(), prev, st["t_now"], 4, 11, call, B, scratch.data_ptr(), valid.data_ptr(), _stream()))
        torch.cuda.synchronize()
        assert not torch.isnan(ref[:, :OD]).any()
        assert torch.equal(_bits(new), _bits(ref)) and torch.equal(_bits(new_v), _bits(ref)) and int(valid) == B
        if B > 200:      # both kinds of goal and (with terminal rows) samples of the episodes that have just ended are among the draws
            assert (idx[2] < 0).any() and (idx[2] >= 0).any()
            assert not terminal or (idx[2] == st["t_now"]).any()


@pytest.mark.parametrize("terminal", [True, False])
def test_draw_relabel_when_every_world_has_just_been_reset(terminal):
    """with terminal rows the finished episodes are sampled; without them nothing can be: the `valid` flavour zero-fills the slot and reports valid[0] = 0"""
    import torch

    from gymnasium_robotics_amd import _native

    L = _native.lib()
    st, args = _ring(0, 3, terminal, True, seed=5)
    B, OW = 4 * N_W, 2 * OD + 3 * 3 + AD + 2
    prev = st["prev"].data_ptr() if terminal else None
    out = torch.full((B, OW), float("nan"), device="cuda:0")
    scratch, valid = torch.zeros(3 * B, dtype=torch.int32, device="cuda:0"), torch.full((1,), -7, dtype=torch.int32, device="cuda:0")
    _native.check(L.grx_her_sample_relabel(ctypes.byref(args(out)), st["start"].data_ptr(), prev, st["t_now"], 4, 11, 0, B, scratch.data_ptr(), valid.data_ptr(), _stream()))
    torch.cuda.synchronize()
    if not terminal:
        assert int(valid) == 0 and torch.equal(out, torch.zeros_like(out))
        return
    idx = [torch.empty(B, dtype=torch.int32, device="cuda:0") for _ in range(3)]
    ref = torch.empty(B, OW, device="cuda:0")
    _native.check(L.grx_her_sample_final(st["start"].data_ptr(), prev, st["term"].data_ptr(), N_W, st["t_now"], T_H, 4, 11, 0, B, *[x.data_ptr() for x in idx], _stream()))
    _native.check(L.grx_her_relabel(ctypes.byref(args(ref, idx)), B, _stream()))
    torch.cuda.synchronize()
    assert int(valid) == B and torch.equal(_bits(out), _bits(ref))


# ------------------------------------------------------------------------------------------------ 3. rollout
def test_fused_tail_rollout_is_the_unfused_rollout(monkeypatch):
    import torch

    from gymnasium_robotics_amd import _native
    from gymnasium_robotics_amd.envs.fetch import FetchVecEnv
    from gymnasium_robotics_amd.her import HerReplay

    n, horizon, steps = 1024, 50, 60      # the smallest batch with cost ordering on

    def make(fused):
        monkeypatch.setenv("GRX_FETCH_FUSED_TAIL", "1" if fused else "0")
        env = FetchVecEnv("FetchPickAndPlace-v4", num_envs=n, device="cuda:0", output="torch", autoreset_mode="same_step")
        assert env._fused == fused and env.balance and env.max_episode_steps == horizon
        env.reset(seed=0)
        env._elapsed[:] = np.arange(n) % horizon      # staggered: every step resets its share of the worlds
        rep = HerReplay(env, horizon=horizon, capacity=4 * n * 4, seed=1, continuous=True)
        assert rep._fused == fused
        rep.begin_episode(env.packed)
        rep.set_episode_start(-env._elapsed)
        return env, rep

    (e1, r1), (e0, r0) = make(True), make(False)
    uploads = {id(r1): 0, id(r0): 0}      # the fused replay takes the reset worlds from the environment's device list: it uploads no mask (a silent fall-back would)
    for rep in (r1, r0):
        monkeypatch.setattr(rep, "_upload_mask", lambda host, rep=rep, f=rep._upload_mask: (uploads.__setitem__(id(rep), uploads[id(rep)] + 1), f(host))[1])
    L = _native.lib()
    g = torch.Generator(device="cuda:0"); g.manual_seed(0)
    order_ref = torch.empty_like(e1.order)
    saw_final = 0
    for step in range(steps):
        a = torch.rand(n, 4, device="cuda:0", generator=g) * 2 - 1
        ema_prev = e1.cost_ema.clone()
        outs = []
        for env, rep in ((e1, r1), (e0, r0)):
            obs, rew, term, trunc, info = env.step(a)
            rep.append(a, env.packed, term | trunc, final_rows=env.final_packed)
            batch = rep.relabel(4 * n, k_future=4)
            outs.append((obs, rew, trunc, info, batch))
        torch.cuda.synchronize()
        (o1, w1, t1, i1, b1), (o0, w0, t0, i0, b0) = outs
        for k in o1:
            assert torch.equal(_bits(o1[k]), _bits(o0[k])), (step, k)
        assert torch.equal(_bits(w1), _bits(w0)) and torch.equal(t1, t0) and torch.equal(i1["is_success"], i0["is_success"]), step
        assert ("final_obs" in i1) == ("final_obs" in i0) == bool(t1.any())
        if "final_obs" in i1:
            saw_final += 1
            assert e1.step_reset_list[1] == int(t1.sum()) and e1.step_reset_list[0][: int(t1.sum())].cpu().tolist() == np.nonzero(t1.numpy())[0].tolist()
            for k in i1["final_obs"]:
                assert torch.equal(_bits(i1["final_obs"][k]), _bits(i0["final_obs"][k])), (step, k)
        assert b1.shape == b0.shape == (4 * n, r1.OW) and torch.equal(_bits(b1), _bits(b0)), step
        for f in ("packed", "final_packed", "status", "qpos", "qvel"):
            assert torch.equal(_bits(getattr(e1, f)), _bits(getattr(e0, f))), (step, f)
        # the order the fused launch left for the next step = grx_order_by_cost_slots on the same costs and the same moving average (see the module docstring)
        _native.check(L.grx_order_by_cost_slots(e1.cost.data_ptr(), ema_prev.data_ptr(), e1.balance_alpha, n, e1._slots_per_xcd, order_ref.data_ptr(), _stream()))
        torch.cuda.synchronize()
        assert torch.equal(e1.order, order_ref) and torch.equal(_bits(e1.cost_ema), _bits(ema_prev)), step
    assert saw_final == steps and r1.t == r0.t == steps
    assert uploads[id(r1)] == 0      # every append of the fused replay marked the boundaries from step_reset_list
    for f in ("episode", "actions", "episode_start", "prev_start", "term_t", "rows"):
        assert torch.equal(_bits(getattr(r1, f)), _bits(getattr(r0, f))), f
    assert (r1.head, r1.size, r1._calls) == (r0.head, r0.size, r0._calls) and np.array_equal(r1._start_host, r0._start_host)
