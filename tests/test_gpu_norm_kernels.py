"""The normaliser kernels (grx_normstat_* of include/grx_capi.h), called through _native on synthetic replay rows and compared with tests/norm_refs.py.

Sums: the terms are exact in fp64, so the device's sums differ from the exactly rounded ones only by the order of summation: |sum_dev - fsum| <= n 2^-53 sum |x| (and
sum x^2 for sumsq).  Refresh: mean / inv_std against the fp64 refresh of the device's own sums, within 2 fp32 ulp (fp64 sqrt and divide are not guaranteed correctly
rounded, plus the final rounding).  Apply: bit for bit the fp32 numpy expression with the device's own mean / inv_std.  Batches sit at the update's partition boundaries
(grx_normstat_geometry: R rows per chunk, G workgroups) and every batch is also read 1, 2 and 3 rows into a larger buffer, which moves its base over the 16-byte phases."""
import ctypes
import functools

import numpy as np
import pytest

import norm_refs as N

pytestmark = pytest.mark.gpu

DIMS = [(1, 1, 1), (4, 2, 2), (25, 3, 4), (153, 7, 20)]      # (obs, goal, act): widths 8, 18, 65 (odd), 349; the last has more columns than a wavefront
EPS, CLIP = 1e-2, 5.0
OFFSETS = (0, 1, 2, 3)


def _lib():
    from gymnasium_robotics_amd import _native

    return _native, _native.lib()


@functools.lru_cache(maxsize=None)
def geometry():
    _, L = _lib()
    R, G = ctypes.c_int(), ctypes.c_int()
    assert L.grx_normstat_geometry(ctypes.byref(R), ctypes.byref(G)) == 0
    return R.value, G.value


def batches():
    R, G = geometry()
    return [1, 63, 64, 65, R - 1, R, R + 1, R * G + 1]


class Block:
    """a zero-filled stat block on the device with views of its public arrays"""

    def __init__(self, od, gd):
        import torch

        _, L = _lib()
        self.od, self.gd, self.D = od, gd, od + gd
        lay = (ctypes.c_int64 * 8)()
        assert L.grx_normstat_layout(od, gd, lay) == 0
        self.lay = [int(v) for v in lay]
        self.raw = torch.zeros(self.lay[7], dtype=torch.uint8, device="cuda:0")
        v = lambda k, n, size, dt: self.raw[self.lay[k]: self.lay[k] + n * size].view(dt)
        self.sum, self.sumsq = v(0, self.D, 8, torch.float64), v(1, self.D, 8, torch.float64)
        self.count, self.skipped = v(2, 1, 8, torch.int64), v(3, 1, 8, torch.int64)
        self.mean, self.inv_std = v(4, self.D, 4, torch.float32), v(5, self.D, 4, torch.float32)

    def update(self, rows, W, valid=None, eps=EPS):
        native, L = _lib()
        native.check(L.grx_normstat_update(self.raw.data_ptr(), rows.data_ptr(), rows.shape[0], W, self.od, self.gd, valid.data_ptr() if valid is not None else None, eps, None))

    def host(self):
        return dict(sum=self.sum.cpu().numpy(), sumsq=self.sumsq.cpu().numpy(), count=int(self.count.item()), skipped=int(self.skipped.item()),
                    mean=self.mean.cpu().numpy(), inv_std=self.inv_std.cpu().numpy())

    def public_bytes(self):
        return self.raw[: self.lay[6]].cpu().numpy().copy()


@functools.lru_cache(maxsize=3)
def case_rows(dims, n):
    """rows [n, W] fp32 of one shape, read-only (regenerated from the seed when the small cache has dropped them)"""
    od, gd, ad = dims
    rng = np.random.default_rng(1000003 * od + n)
    rows = (0.5 + 2.0 * rng.standard_normal((n, N.row_width(od, gd, ad)))).astype(np.float32)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def case_sums(dims, n):
    return N.batch_sums(case_rows(dims, n), dims[0], dims[1])


def case(dims, n):
    """(rows, reference sums) of one shape: the reference is computed once and shared by every test that reads it"""
    return case_rows(dims, n), case_sums(dims, n)


def shifted(rows, k, pad=4):
    """a device view of `rows` that starts k rows into a larger buffer (the rows around it hold a sentinel that would wreck every sum)"""
    import torch

    n, W = rows.shape
    buf = torch.full((n + pad, W), 3.0e30, dtype=torch.float32, device="cuda:0")
    view = buf[k: k + n]
    view.copy_(torch.from_numpy(rows))
    assert view.is_contiguous()
    return buf, view


def check_sums(h, ref, n_terms):
    s, q, a, kept, skipped = ref
    print("max |sum - fsum| / bound:", float(np.max(np.abs(h["sum"] - s) / np.maximum(N.sum_bound(a, n_terms), 1e-300))) if n_terms > 1 else 0.0)
    assert (np.abs(h["sum"] - s) <= N.sum_bound(a, n_terms)).all()
    assert (np.abs(h["sumsq"] - q) <= N.sum_bound(q, n_terms)).all()
    assert h["count"] == kept and h["skipped"] == skipped


def check_refresh(h, eps=EPS):
    mean, inv = N.refresh(h["sum"], h["sumsq"], h["count"], eps)
    assert N.ulp_distance(h["mean"], mean).max() <= 2, (h["mean"], mean)
    assert N.ulp_distance(h["inv_std"], inv).max() <= 2, (h["inv_std"], inv)


def same_bits(dev, ref):
    """fp32 arrays equal bit for bit, NaNs at the same places (their payloads are not compared)"""
    dev, ref = np.ascontiguousarray(dev, np.float32), np.ascontiguousarray(ref, np.float32)
    nd, nr = np.isnan(dev), np.isnan(ref)
    return dev.shape == ref.shape and (nd == nr).all() and (dev.view(np.uint32)[~nd] == ref.view(np.uint32)[~nd]).all()


# ------------------------------------------------------------------ update
@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("which", range(8))
def test_update_sums_count_and_refresh(dims, which):
    import torch

    n = batches()[which]
    od, gd, ad = dims
    rows, ref = case(dims, n)
    W = rows.shape[1]
    first = None
    for k in OFFSETS:
        buf, view = shifted(rows, k)
        blk = Block(od, gd)
        blk.update(view, W)
        h = blk.host()
        check_sums(h, ref, n)
        check_refresh(h)
        if first is None:
            first = h
        # the partition does not depend on where the rows lie: the same bits at every offset
        assert (h["sum"].view(np.uint64) == first["sum"].view(np.uint64)).all() and (h["sumsq"].view(np.uint64) == first["sumsq"].view(np.uint64)).all()
        del buf, view
    torch.cuda.synchronize()


def test_fresh_block_is_the_identity():
    blk = Block(25, 3)
    native, L = _lib()
    native.check(L.grx_normstat_refresh(blk.raw.data_ptr(), 25, 3, EPS, None))
    h = blk.host()
    assert h["count"] == 0 and (h["mean"] == 0).all() and (h["inv_std"] == 1).all()


def test_large_mean_small_spread_needs_fp64():
    """mean 1000, spread 0.01 at R G + 1 rows: an fp32 accumulator is off by far more than the bound (shown on the host), the device is inside it"""
    R, G = geometry()
    dims, n = (25, 3, 4), R * G + 1
    od, gd, ad = dims
    rng = np.random.default_rng(5)
    rows = (1000.0 + 0.01 * rng.standard_normal((n, N.row_width(*dims)))).astype(np.float32)
    ref = N.batch_sums(rows, od, gd)
    x = rows[:, N.tracked_columns(od, gd)]
    naive32 = np.cumsum(x, axis=0, dtype=np.float32)[-1].astype(np.float64)
    assert (np.abs(naive32 - ref[0]) > N.sum_bound(ref[2], n)).all()
    _, view = shifted(rows, 1)
    blk = Block(od, gd)
    blk.update(view, rows.shape[1])
    h = blk.host()
    check_sums(h, ref, n)
    check_refresh(h)
    # what it is for: the variance survives.  std ~ 0.01 = eps here, so compare the variance of the sums directly
    var = h["sumsq"] / n - (h["sum"] / n) ** 2
    np.testing.assert_allclose(var, np.var(x.astype(np.float64), axis=0), rtol=1e-3)


@pytest.mark.parametrize("dims", [(25, 3, 4), (153, 7, 20)])
def test_three_updates_accumulate_and_repeat_bit_for_bit(dims):
    R, G = geometry()
    od, gd, ad = dims
    sizes = (R + 1, 257, 3 * R - 1)
    parts = [case(dims, n)[0] for n in sizes]
    W = parts[0].shape[1]
    ref = N.batch_sums(np.concatenate(parts), od, gd)      # one reference over the concatenation
    views = [shifted(p, 1 + i) for i, p in enumerate(parts)]
    blocks = [Block(od, gd), Block(od, gd)]
    for blk in blocks:
        for _, v in views:
            blk.update(v, W)
    a, b = blocks[0].host(), blocks[1].host()
    check_sums(a, ref, sum(sizes))
    check_refresh(a)
    assert (a["sum"].view(np.uint64) == b["sum"].view(np.uint64)).all() and (a["sumsq"].view(np.uint64) == b["sumsq"].view(np.uint64)).all()
    assert (blocks[0].public_bytes() == blocks[1].public_bytes()).all()


def test_valid_word_is_read_on_the_device():
    import torch

    dims = (25, 3, 4)
    od, gd, ad = dims
    R, G = geometry()
    rows, ref = case(dims, R + 1)
    other = case(dims, 65)[0]
    W = rows.shape[1]
    _, v1 = shifted(rows, 1)
    _, v2 = shifted(other, 2)
    blk = Block(od, gd)
    blk.update(v1, W)      # valid = NULL counts the batch
    assert blk.host()["count"] == R + 1
    before = blk.raw.cpu().numpy().copy()
    zero, some = torch.zeros(1, dtype=torch.int32, device="cuda:0"), torch.full((1,), 65, dtype=torch.int32, device="cuda:0")
    blk.update(v2, W, valid=zero)
    assert (blk.raw.cpu().numpy() == before).all()      # the whole block, workspace included
    blk.update(v2, W, valid=some)
    h = blk.host()
    assert h["count"] == R + 1 + 65
    both = N.batch_sums(np.concatenate([rows, other]), od, gd)
    check_sums(h, both, R + 1 + 65)
    fresh = Block(od, gd)
    fresh.update(v2, W, valid=zero)      # also on a block that has seen nothing: not even the refresh runs, the zero-filled allocation stays as it is
    assert not fresh.raw.cpu().numpy().any()


@pytest.mark.parametrize("dims", DIMS)
def test_rows_with_non_finite_tracked_values_are_skipped(dims):
    od, gd, ad = dims
    R, G = geometry()
    n = 2 * R + 5
    rows = case(dims, n)[0].copy()
    W = rows.shape[1]
    tracked = N.tracked_columns(od, gd)
    untracked = np.setdiff1d(np.arange(W), tracked)
    planted = [0, n - 1, R - 1, R, 2 * R - 1, 2 * R]      # first, last, and both sides of two chunk boundaries
    values = [np.nan, np.inf, -np.inf, np.nan, -np.inf, np.inf]
    for i, (r, v) in enumerate(zip(planted, values)):
        rows[r, tracked[(i * 7) % len(tracked)]] = v
    rows[R, tracked[-1]] = np.inf      # two bad values in one row still skip it once
    for r in (1, R - 2, R + 1, n - 2):      # untracked columns of other rows: achieved, action, reward, obs_t+1, ..., success
        rows[r, untracked] = np.nan
    ref = N.batch_sums(rows, od, gd)
    assert ref[3] == n - len(planted) and ref[4] == len(planted)
    clean = N.batch_sums(np.delete(rows, planted, axis=0), od, gd)      # the sums are those of the remaining rows: a condition, not a tolerance
    assert (clean[0] == ref[0]).all() and (clean[1] == ref[1]).all() and clean[3] == ref[3]
    for k in (0, 3):
        _, view = shifted(rows, k)
        blk = Block(od, gd)
        blk.update(view, W)
        h = blk.host()
        assert h["skipped"] == len(planted) and h["count"] == n - len(planted)
        assert np.isfinite(h["sum"]).all() and np.isfinite(h["sumsq"]).all()
        check_sums(h, ref, n - len(planted))
        check_refresh(h)


# ------------------------------------------------------------------ apply
def spiked(rows, seed, dims=None):
    """rows with values far beyond the clip, NaN, +-inf, signed zeros and a denormal scattered over every kind of column; with `dims` and at least 8 replay rows also one of
    each planted where it is known to be normalised (obs_t, goal) or copied (action, reward)"""
    rng = np.random.default_rng(seed)
    out = rows.copy()
    flat = out.reshape(-1)
    k = min(max(4, flat.size // 50), flat.size)
    idx = rng.choice(flat.size, size=k, replace=False)
    vals = np.array([1e6, -1e6, np.nan, np.inf, -np.inf, 40.0, -40.0, 0.0, -0.0, 1e-42], np.float32)
    flat[idx] = vals[np.arange(k) % len(vals)]
    if dims is not None and len(out) >= 8:
        od, gd, ad = dims
        out[1, 0], out[2, 0], out[3, 0], out[4, od + gd], out[5, od + gd], out[6, od + 2 * gd], out[7, od + 2 * gd + ad] = 1e6, -1e6, np.nan, np.inf, -np.inf, np.nan, 1e6
    return out


def same_bits_dev(out, want):
    """device tensors equal bit for bit, NaNs at the same places"""
    import torch

    return bool(((out.view(torch.int32) == want.view(torch.int32)) | (torch.isnan(out) & torch.isnan(want))).all())


def trained_block(dims):
    od, gd, ad = dims
    rows, _ = case(dims, 65)
    _, v = shifted(rows, 0)
    blk = Block(od, gd)
    blk.update(v, rows.shape[1])
    return blk


@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("which", range(8))
def test_apply_batch_is_the_fp32_expression_bit_for_bit(dims, which):
    import torch

    native, L = _lib()
    n = batches()[which]
    od, gd, ad = dims
    W = N.row_width(*dims)
    rows = spiked(case_rows(dims, n), which, dims)
    blk = trained_block(dims)
    h = blk.host()
    want = N.apply_batch(rows, h["mean"], h["inv_std"], od, gd, ad, CLIP)
    passthrough = np.setdiff1d(np.arange(W), np.concatenate([np.arange(od + 2 * gd), od + 2 * gd + ad + 1 + np.arange(od + gd)]))
    assert len(passthrough) == ad + 2 and same_bits(want[:, passthrough], rows[:, passthrough])
    if n >= 8:
        assert want[1, 0] == CLIP and want[2, 0] == -CLIP and np.isnan(want[3, 0]) and want[4, od + gd] == CLIP and want[5, od + gd] == -CLIP
        assert np.isnan(want[6, od + 2 * gd]) and want[7, od + 2 * gd + ad] == np.float32(1e6)
    want_dev, rows_dev = torch.from_numpy(want).cuda(), torch.from_numpy(rows).cuda()
    for k in OFFSETS:
        _, src = shifted(rows, k)
        ko = (k + which) % 4      # the same 16-byte phase as the source for some offsets, another for others
        obuf = torch.full((n + 4, W), -7.0, dtype=torch.float32, device="cuda:0")
        out = obuf[ko: ko + n]
        native.check(L.grx_normstat_apply_batch(blk.raw.data_ptr(), src.data_ptr(), n, W, od, gd, ad, CLIP, out.data_ptr(), None))
        assert same_bits_dev(out, want_dev), (dims, n, k)
        assert same_bits_dev(src, rows_dev)      # the source is not written
        assert bool((obuf[:ko] == -7.0).all()) and bool((obuf[ko + n:] == -7.0).all())
        native.check(L.grx_normstat_apply_batch(blk.raw.data_ptr(), src.data_ptr(), n, W, od, gd, ad, CLIP, src.data_ptr(), None))      # in place
        assert same_bits_dev(src, want_dev), (dims, n, k, "in place")
    assert same_bits(out.cpu().numpy(), want)      # once through the host as well


@pytest.mark.parametrize("dims", DIMS)
def test_apply_packed_is_the_actor_input(dims):
    import torch

    native, L = _lib()
    od, gd, ad = dims
    D, PW = od + gd, od + 2 * gd + 2
    blk = trained_block(dims)
    h = blk.host()
    for n in (1, 63, 257, 4099):
        rng = np.random.default_rng(n)
        packed = spiked((0.5 + 2.0 * rng.standard_normal((n, PW))).astype(np.float32), n)
        want = N.apply_packed(packed, h["mean"], h["inv_std"], od, gd, CLIP)
        _, src = shifted(packed, n % 4)
        obuf = torch.full((n + 2, D), -7.0, dtype=torch.float32, device="cuda:0")
        out = obuf[1: 1 + n]
        native.check(L.grx_normstat_apply_packed(blk.raw.data_ptr(), src.data_ptr(), n, PW, od, gd, CLIP, out.data_ptr(), None))
        assert same_bits(out.cpu().numpy(), want), (dims, n)
        guard = obuf.cpu().numpy()
        assert (guard[0] == -7.0).all() and (guard[-1] == -7.0).all()
