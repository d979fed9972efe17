"""Plain numpy / math.fsum reference of the observation and goal normaliser (include/grx_capi.h grx_normstat_*, include/grx_norm.h, her.Normalizer).

The sums are the exactly rounded ones (math.fsum over the fp64-converted values and over their fp64 squares, which are exact), the refresh is in fp64, the apply in fp32
in the stated order.  Nothing here imports the package: test_cpu_norm_refs.py checks these functions against an independent two-pass mean / variance, the GPU tests check
the kernels against them.
"""
import math

import numpy as np


def row_width(od, gd, ad):
    return 2 * od + 3 * gd + ad + 2


def tracked_columns(od, gd):
    """columns of a replay row [obs_t | achieved_t | goal | action_t | reward | obs_t+1 | achieved_t+1 | success] that feed the statistics: obs_t, then the goal"""
    return np.concatenate([np.arange(od), od + gd + np.arange(gd)])


def kept_rows(rows, od, gd):
    """mask of the rows that count: every tracked value finite (other columns are not looked at)"""
    return np.isfinite(rows[:, tracked_columns(od, gd)]).all(axis=1)


class Stats:
    """the public part of a stat block"""

    def __init__(self, D):
        self.sum, self.sumsq = np.zeros(D, np.float64), np.zeros(D, np.float64)
        self.count, self.skipped = 0, 0
        self.abs_sum = np.zeros(D, np.float64)      # sum |x| and the number of terms: what the summation-order bound of the GPU tests is made of
        self.terms = 0


def fsum_columns(x64):
    return np.array([math.fsum(col) for col in np.ascontiguousarray(x64.T).tolist()], np.float64)


def batch_sums(rows, od, gd):
    """(sum, sumsq, sum |x|, kept, skipped) of one batch: exactly rounded column sums over the rows that count"""
    keep = kept_rows(rows, od, gd)
    x = rows[keep][:, tracked_columns(od, gd)].astype(np.float64)
    return fsum_columns(x), fsum_columns(x * x), np.abs(x).sum(axis=0), int(keep.sum()), int((~keep).sum())      # sum |x| only scales a bound: any rounding will do


def update(st, rows, od, gd, valid=None):
    """one update call: a zero `valid` word changes nothing"""
    if valid is not None and int(valid) == 0:
        return st
    s, q, a, kept, skipped = batch_sums(rows, od, gd)
    st.sum = st.sum + s
    st.sumsq = st.sumsq + q
    st.abs_sum = st.abs_sum + a
    st.count += kept
    st.skipped += skipped
    st.terms += kept
    return st


def refresh(total, sumsq, count, eps):
    """(mean fp32, inv_std fp32) of the running sums, in fp64: mean = sum / count, var = sumsq / count - mean^2, std = sqrt(max(eps^2, var)); count 0: (0, 1)"""
    total, sumsq = np.asarray(total, np.float64), np.asarray(sumsq, np.float64)
    if count == 0:
        return np.zeros(len(total), np.float32), np.ones(len(total), np.float32)
    n = np.float64(count)
    mean = total / n
    var = sumsq / n - mean * mean
    std = np.sqrt(np.maximum(np.float64(eps) * np.float64(eps), var))
    return mean.astype(np.float32), (np.float64(1.0) / std).astype(np.float32)


def normalize(x, mean, inv_std, clip):
    """fp32, in this order: y = (x - mean) * inv_std, then clipped to [-clip, clip]; a NaN stays a NaN, +-inf clips"""
    x, mean, inv_std, clip = np.asarray(x, np.float32), np.asarray(mean, np.float32), np.asarray(inv_std, np.float32), np.float32(clip)
    with np.errstate(invalid="ignore", over="ignore"):
        y = ((x - mean).astype(np.float32) * inv_std).astype(np.float32)
        y = np.where(y < -clip, -clip, y)
        y = np.where(y > clip, clip, y)
    return y.astype(np.float32)


def apply_batch(rows, mean, inv_std, od, gd, ad, clip):
    """replay rows with obs_t / obs_t+1 (observation statistics) and achieved_t / goal / achieved_t+1 (goal statistics) normalised, the rest copied bit for bit"""
    rows = np.asarray(rows, np.float32)
    out = rows.copy()
    mo, so, mg, sg = mean[:od], inv_std[:od], mean[od:], inv_std[od:]
    o2 = od + 2 * gd + ad + 1
    out[:, :od] = normalize(rows[:, :od], mo, so, clip)
    out[:, od: od + gd] = normalize(rows[:, od: od + gd], mg, sg, clip)
    out[:, od + gd: od + 2 * gd] = normalize(rows[:, od + gd: od + 2 * gd], mg, sg, clip)
    out[:, o2: o2 + od] = normalize(rows[:, o2: o2 + od], mo, so, clip)
    out[:, o2 + od: o2 + od + gd] = normalize(rows[:, o2 + od: o2 + od + gd], mg, sg, clip)
    return out


def apply_packed(packed, mean, inv_std, od, gd, clip):
    """[n, od + gd] = [norm(obs) | norm(desired)] of packed env rows [obs | achieved | desired | reward | success]"""
    packed = np.asarray(packed, np.float32)
    return np.concatenate([normalize(packed[:, :od], mean[:od], inv_std[:od], clip), normalize(packed[:, od + gd: od + 2 * gd], mean[od:], inv_std[od:], clip)], axis=1)


def sum_bound(abs_sum, terms):
    """|any-order fp64 sum - exactly rounded sum| of `terms` exact terms: terms * 2^-53 * sum |x|"""
    return terms * 2.0 ** -53 * np.asarray(abs_sum, np.float64)


def ulp_distance(a, b):
    """distance of two finite fp32 arrays in units in the last place (the bit patterns mapped to a monotonic integer line, so a sign change counts too)"""
    def line(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)

    return np.abs(line(a) - line(b))
