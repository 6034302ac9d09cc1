"""numpy restatement of the single-pulse search (include/fxcorr.h fxc_boxcar_search) with exactly its order of
operations, the hooks of the mutations in tests/test_boxcar_host.py, a float64 truth, and the inputs both test modules use.
Nothing here imports the library."""
import numpy as np

import dedisperse_ref

SEGMENT = 256          # samples of a segment sum, segment sums of a group sum
MAX_J = 12
ROOTS = np.sqrt(np.float64(2.0) ** np.arange(MAX_J + 1))      # r_j, the table of 13 entries

PULSE_WIDTH, PULSE_HEIGHT = 8, 0.25
PULSE_J = 3


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _sequential(a):
    """the sums of the rows of a [n, k] float64 array, each from +0 in ascending order (accumulate is strictly sequential)"""
    return np.add.accumulate(np.concatenate([np.zeros((a.shape[0], 1)), a], axis=1), axis=1)[:, -1]


def _lines(v, k):
    """a float64 vector as lines of k, the last filled up with +0: adding +0 changes no bit of a sum that started from +0"""
    n = -(-v.size // k)
    out = np.zeros(n * k)
    out[:v.size] = v
    return out.reshape(n, k)


def tree_sum(terms, counted, drop="select"):
    """segments of 256 from t = 0, 256 segment sums to a group sum, the group sums in ascending order.  A sample that does not
    count is selected away (its term replaced by +0, which changes no bit); drop="multiply" is the mutation"""
    with np.errstate(all="ignore"):
        terms = np.where(counted, terms, 0.0) if drop == "select" else terms * counted
        groups = _sequential(_lines(_sequential(_lines(terms, SEGMENT)), SEGMENT))
        return float(_sequential(groups.reshape(1, -1))[0])


def row_stats(x, clip=3.0, clip_iters=2, clip_against="this round", drop="select"):
    """-> (m, std, n, degenerate) of one row.  clip_against="previous round" and drop="multiply" are mutations"""
    xd = np.asarray(x).astype(np.float64)
    counted = np.ones(xd.size, bool)
    rounds = 0 if clip == 0 else int(clip_iters)
    c2 = np.float64(clip) * np.float64(clip)
    m_before = None
    with np.errstate(all="ignore"):
        for r in range(rounds + 1):
            n = int(counted.sum())
            m = np.float64(tree_sum(xd, counted, drop)) / np.float64(n)
            if n < 2:
                return float(m), 0.0, n, True
            e = xd - m
            v = np.float64(tree_sum(e * e, counted, drop)) / np.float64(n - 1)
            if r < rounds:
                limit = c2 * v
                ec = e if clip_against == "this round" or m_before is None else xd - m_before
                counted = ec * ec <= limit
                m_before = m
        if v == 0:
            return float(m), 0.0, n, True
        return float(m), float(np.sqrt(v)), n, False


def levels(y, j_hi, child=0, in_place=False, tile=None):
    """-> [L_0 .. L_j_hi] of the float32 row y, L_j of n_t - 2^j + 1 entries (none where the width does not fit).  The mutations:
    child = +1 / -1 moves the second child, in_place reads the second child after it was overwritten (one buffer, walked so that
    t + 2^(j-1) is done before t), tile cuts the row into pieces whose halo is zeros"""
    y = np.asarray(y, np.float32)
    n_t = y.size
    if tile is not None:
        parts = [levels(np.concatenate([y[a:a + tile], np.zeros(1 << j_hi, np.float32)]), j_hi) for a in range(0, n_t, tile)]
        return [np.concatenate([p[j][:tile] for p in parts])[:n_t - (1 << j) + 1] if (1 << j) <= n_t else None for j in range(j_hi + 1)]
    out = [y]
    for j in range(1, j_hi + 1):
        if (1 << j) > n_t:
            out.append(None)
            continue
        prev, n = out[-1], n_t - (1 << j) + 1
        h = (1 << (j - 1)) + child
        if in_place:
            cur = prev.copy()
            for t in range(n - 1, -1, -1):
                cur[t] = cur[t] + cur[t + h]
            out.append(cur[:n])
        else:
            second = np.concatenate([prev, np.zeros(2, np.float32)])[h:h + n]
            out.append(prev[:n] + second)
        assert out[-1].dtype == np.float32
    return out


def search_row(x, j_lo, j_hi, block, clip=3.0, clip_iters=2, subtract_mean=True, use_root=True, ties="narrowest, earliest",
               starts_of_blocks="n_t - 2^j_lo + 1", stats=None, **level_hooks):
    """one row -> (snr [n_blk] float32, width int32, time int32, (m, std, n)).  The keyword arguments past clip_iters are the
    mutations' hooks"""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 1 and 0 <= j_lo <= j_hi <= MAX_J and (1 << j_lo) <= x.size
    n_t = x.size
    m, std, n, degenerate = stats if stats is not None else row_stats(x, clip, clip_iters)
    n_starts = n_t - (1 << j_lo) + 1 if starts_of_blocks == "n_t - 2^j_lo + 1" else n_t
    n_blk = -(-n_starts // block)
    first = (np.arange(n_blk, dtype=np.int64) * block).astype(np.int32)
    if degenerate:
        return np.zeros(n_blk, np.float32), np.full(n_blk, j_lo, np.int32), first, (m, std, n)
    y = (x.astype(np.float64) - (np.float64(m) if subtract_mean else 0.0)).astype(np.float32)
    lv = levels(y, j_hi, **level_hooks)
    best = best_j = best_t = None
    with np.errstate(all="ignore"):
        for j in range(j_lo, j_hi + 1):
            if (1 << j) > n_t:
                break
            den = np.float64(std) * (ROOTS[j] if use_root else np.float64(1.0))
            snr = (lv[j].astype(np.float64) / den).astype(np.float32)
            grid = np.full(n_blk * block, -np.inf, np.float32)      # a start that does not exist never replaces
            k = min(snr.size, n_starts)
            grid[:k] = snr[:k]
            grid = grid.reshape(n_blk, block)
            if ties == "latest start":
                at = block - 1 - np.argmax(grid[:, ::-1], axis=1)
            else:
                at = np.argmax(grid, axis=1)                        # the first of the largest
            top = grid[np.arange(n_blk), at]
            if best is None:
                best, best_j, best_t = top.copy(), np.full(n_blk, j, np.int32), (first + at).astype(np.int32)
                continue
            better = top >= best if ties == "widest width" else top > best
            best = np.where(better, top, best)
            best_j = np.where(better, np.int32(j), best_j).astype(np.int32)
            best_t = np.where(better, first + at, best_t).astype(np.int32)
    return best, best_j, best_t, (m, std, n)


def search(ts, widths=(0, 8), block=64, clip=3.0, clip_iters=2, **hooks):
    """[..., n_t] float32 -> (snr, width, time) of shape ts.shape[:-1] + (n_blk,) and stats float64 [..., 3]"""
    ts = np.asarray(ts)
    rows = ts.reshape(-1, ts.shape[-1])
    res = [search_row(r, widths[0], widths[1], block, clip, clip_iters, **hooks) for r in rows]
    lead = ts.shape[:-1]
    return (np.stack([r[0] for r in res]).reshape(lead + (-1,)), np.stack([r[1] for r in res]).reshape(lead + (-1,)),
            np.stack([r[2] for r in res]).reshape(lead + (-1,)), np.array([r[3] for r in res], np.float64).reshape(lead + (3,)))


def truth(x, j, clip=3.0, clip_iters=2):
    """one row in float64 with exact means -> (m, std, n, snr_j of every start): the rounds' sums by math.fsum, the boxcar from
    differences of an extended-precision running sum"""
    import math
    xd = np.asarray(x).astype(np.float64)
    counted = np.ones(xd.size, bool)
    rounds = 0 if clip == 0 else int(clip_iters)
    for r in range(rounds + 1):
        n = int(counted.sum())
        m = math.fsum(xd[counted]) / n
        v = math.fsum((xd[counted] - m) ** 2) / (n - 1)
        if r < rounds:
            counted = (xd - m) ** 2 <= clip * clip * v
    std = math.sqrt(v)
    run = np.concatenate([[0], np.cumsum((xd - m).astype(np.longdouble))])
    w = 1 << j
    return m, std, n, ((run[w:] - run[:-w]) / (std * math.sqrt(w))).astype(np.float64)


# -- inputs -------------------------------------------------------------------------------------------------------------------------
def loud_rows(rng, n_rows, n_t, spikes=True):
    """seeded noise on a ramp, every row on a scale and an offset of its own so that the mean matters, and a few samples at 10 .. 50
    standard deviations so that the clipping rounds differ"""
    scale = 0.5 + 4.0 * rng.random((n_rows, 1))
    offset = 20.0 * (rng.random((n_rows, 1)) - 0.3) * scale
    x = offset + scale * (rng.standard_normal((n_rows, n_t)) + 0.5 * np.arange(n_t) / n_t)
    if spikes and n_t >= 16:
        for r in range(n_rows):
            at = rng.choice(n_t, size=min(6, n_t // 8), replace=False)
            x[r, at] += scale[r] * rng.uniform(10.0, 50.0, at.size)
    return x.astype(np.float32)


def tie_row(n_t):
    """small integers with exact ties, n_t >= 256: a background of +1, -1 in turn; two equal spikes of 8 at 77 and 82 -- a tie across
    starts --; a plateau of four 4s from 87, whose sum of 16 at width 4 gives 16 / (2 std), the bits of the spikes' 8 / std at
    width 1 -- a tie across widths, all inside the block 74 .. 110 of a block size of 37.  The second half of the row is the first
    negated, so the mean is exactly 0 before and after every clipping round, and every level holds small integers"""
    assert n_t >= 256
    half = np.where(np.arange(n_t // 2) % 2 == 0, 1.0, -1.0).astype(np.float32)
    half[[77, 82]] = 8.0
    half[87:91] = 4.0
    return np.concatenate([half, -half, np.zeros(n_t % 2, np.float32)])


def wide_pulse_case(seed):
    """dedisperse_ref.pulse_case's noise (8 chunks x 2 series x 128 bins x 64 channels, chi-square 32) with a pulse of 8 samples of
    height 0.25 in every channel of series 1 along the DM 10 sweep from t0 = 300 -> (power, shifts, the dedispersed series [2, 9, 637])"""
    rng = np.random.default_rng(seed)
    ref = dedisperse_ref
    shifts = ref.wide_shifts()
    power = (rng.chisquare(32, (ref.PULSE_CHUNKS, ref.PULSE_SERIES, ref.PULSE_TBIN, ref.WIDE_NCHAN)) / 32.0).astype(np.float32)
    for k in range(ref.WIDE_NCHAN):
        for i in range(PULSE_WIDTH):
            t = ref.PULSE_T0 + i + int(shifts[ref.PULSE_DM_INDEX, k])
            power[t // ref.PULSE_TBIN, ref.PULSE_SERIES_AT, t % ref.PULSE_TBIN, k] += np.float32(PULSE_HEIGHT)
    return power, shifts, ref.dedisperse(power, shifts)
