"""Numpy reference of pcp_icp_trim_keys (include/pcp.h, I3), written from the contract text, not
from the kernel:

  * a key is valid when it is not INT64_MAX; b = key >> 32 as uint32; m = number of valid keys;
  * r = floor(float64(frac) * float64(m - 1)) with frac the fp32 value the C entry receives;
    sel = the r-th smallest b of a stable sort in unsigned order (0 when m == 0);
  * m2 = mult * mult, c = m2 * as_float(sel), f2 = d_floor * d_floor in float32 (numpy rounds each
    float32 operation to nearest and never contracts); cut = f2 when c is NaN, else max(c, f2);
  * a key is kept iff it is valid and as_float(b) <= cut (False for a NaN pattern); a kept key is
    unchanged, every other key is INT64_MAX;
  * stats = [m, kept, sel, bits of cut].
"""
import numpy as np

NO_KEY = np.iinfo(np.int64).max
_ERR = dict(invalid="ignore", over="ignore", under="ignore")


def high_words(keys):
    return (np.asarray(keys).astype(np.uint64) >> np.uint64(32)).astype(np.uint32)


def make_keys(high, low):
    """int64 keys of uint32 high words (d2 bits) and low words (target indices)."""
    k = (np.asarray(high).astype(np.uint64) << np.uint64(32)) | np.asarray(low).astype(np.uint64)
    return k.view(np.int64)


def rank(frac, m):
    """The contract's r for m >= 1 valid keys."""
    return int(np.floor(np.float64(np.float32(frac)) * np.float64(m - 1)))


def select(keys, frac):
    """(m, sel): the number of valid keys and the r-th smallest high word (0 when m == 0)."""
    keys = np.asarray(keys).view(np.int64)
    b = high_words(keys[keys != NO_KEY])
    if b.size == 0:
        return 0, 0
    return int(b.size), int(np.sort(b, kind="stable")[rank(frac, b.size)])


def cut_of(sel, mult, d_floor):
    """The fp32 cut of a selected bit pattern."""
    with np.errstate(**_ERR):
        m2 = np.float32(mult) * np.float32(mult)
        c = m2 * np.array([sel], dtype=np.uint32).view(np.float32)[0]
        f2 = np.float32(d_floor) * np.float32(d_floor)
    if np.isnan(c) or not c > f2:
        return np.float32(f2)
    return np.float32(c)


def keep_mask(keys, cut):
    keys = np.asarray(keys).view(np.int64)
    with np.errstate(**_ERR):
        return (keys != NO_KEY) & (high_words(keys).view(np.float32) <= np.float32(cut))


def trim(keys, frac, mult=1.0, d_floor=0.0):
    """(keys_out int64, stats uint64[4]) of the contract."""
    keys = np.ascontiguousarray(np.asarray(keys).view(np.int64))
    m, sel = select(keys, frac)
    cut = cut_of(sel, mult, d_floor)
    keep = keep_mask(keys, cut)
    out = np.where(keep, keys, np.int64(NO_KEY))
    stats = np.array([m, int(keep.sum()), sel, int(np.array([cut], dtype=np.float32).view(np.uint32)[0])],
                     dtype=np.uint64)
    return out, stats


def cluttered_queries(q, T_true, share=0.25, z_band=(0.15, 0.45), half=24.0, seed=5):
    """The partial-overlap scene of the trimmed-ICP tests: the last `share` of the queries q
    ((n, 3) float32, in the query frame) are replaced by clutter that has no counterpart in the
    target -- points uniform over [-half, half]^2 at heights z_band in the target frame, mapped
    into the query frame by T_true^-1 in float64 -- and the result is shuffled."""
    rng = np.random.default_rng(seed)
    q = np.asarray(q, dtype=np.float32)
    nout = int(share * len(q))
    xy = rng.uniform(-half, half, (nout, 2))
    z = rng.uniform(z_band[0], z_band[1], nout)
    c = np.concatenate([xy, z[:, None]], 1).astype(np.float32).astype(np.float64)
    cq = ((c - T_true[:3, 3]) @ T_true[:3, :3]).astype(np.float32)
    q2 = np.concatenate([q[: len(q) - nout], cq], 0)
    return np.ascontiguousarray(q2[rng.permutation(len(q2))])
