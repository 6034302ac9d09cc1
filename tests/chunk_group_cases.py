"""Integrations in which an X-engine sums more than one chunk into a raw row.

For three and more antennas, and on every plan with autos, an untracked fx_accumulate hands the spectra of a pass to an X-engine
kernel that writes one raw float32 row per *chunk group* of ``cg`` chunks (h_launch.h::xengine_group, h_run.h::autos_group):

    cg = max(1, min(fused_unit, ceil(nc / groups)))        groups = max(1, x_resident / cols)

with ``nc`` the chunks of the pass, ``fused_unit = min(1024 / n_pts, 64)`` the chunks a float32 row may hold, ``cols`` the
workgroups a row takes and ``x_resident`` the workgroups of the kernel the device holds at once.  An MI355X holds thousands, so a
call of a few chunks has ``cg`` = 1.  Python cannot see ``x_resident``; the cases here therefore take their chunk counts from the
device's CU count and an *upper bound* of it (``per_cu_bound``): 32 one-wave workgroups per CU, the cap of
h_build.h::xengine_resident, for xengine_kernel<A>, its AUTOS form and xengine_block_kernel; what 160 KiB of LDS per CU hold of
XMfmaGeo<T>::kLdsBytes for xengine_mfma_kernel<T> (4, 4, 3, 2 for T = 1 .. 4).  With ``groups_max = bound * cu_count / cols`` a
call of

    n >= 2 * groups_max + 1,   n > fused_unit,   n prime                                                  (``call_chunks``)

chunks has ``cg`` >= 3 whatever the occupancy is, more than one group whatever ``cg`` is, and a last group shorter than ``cg``
for every ``cg`` the device can choose (2 .. fused_unit: none of them divides a prime above fused_unit).  Every case calls
fx_accumulate twice, ``SHORT`` chunks and then those ``n``, so that an integration spans calls with different groupings.

Channel counts: ``n * nchan`` is about ``2 * bound * cu_count * (bins of a column)`` at every channel count, so the input does
not shrink with the channel count; the cases take the largest one at which ``2 * groups_max + 1`` still reaches fused_unit + 1
on 256 CUs (fewer chunks for the oracle's loops), 4096 channels once (a real array's shape: four groups of 17 chunks on an
MI355X), 32 channels once (part of a wave) and 4096 once more for the fused F stage.

``test_chunk_groups_host.py`` proves these claims from the model below for 64, 128, 256 and 304 CUs, and
``test_gpu_chunk_groups.py`` runs the cases against the float64 oracle."""
import collections
import functools

import numpy as np

Case = collections.namedtuple("Case", "id kernel n_ant nchan n_pts ntaps tail autos rot path passes")

BW = 2.4e6
FREQ = 1.4204e9
TAU_ROT = 3.7e-7                 # the rot table's delay (cases with ``rot``)
SHORT = 2                        # chunks of every case's first fx_accumulate call
CU_COUNTS = (64, 128, 256, 304)  # the devices the host test models
INPUT_CAP = 300 * 10 ** 6        # bytes of a case's samples
K_ROW_SPECTRA = 1024             # h_launch.h::kRowSpectra
X_THREADS = 64                   # k_finish.h::kXThreads
X_BLOCK = 8                      # k_finish.h::kXB
ONE_WAVE_PER_CU = 32             # h_build.h::xengine_resident: 4 SIMDs x 8 waves at the most
LDS_PER_CU = 160 << 10
MFMA_PITCH = 17                  # k_xmfma.h: XMfmaGeo<T>::kPitch = kCH + 1, kCH = 16
MFMA_COLUMN = 16
SUBSET_FROM = 49                 # antennas from which the oracle takes a subset of the baselines (``oracle_pairs``)


def _case(kernel, n_ant, nchan, n_pts, ntaps, tail=0, rot=False, autos=False, path="tiled", passes=False):
    name = "%s-%dx%dx%d%s" % (kernel, n_ant, nchan, n_pts, "-passes" if passes else "")
    return Case(name, kernel, n_ant, nchan, n_pts, ntaps, tail, autos, rot, path, passes)


CASES = [
    # xengine_mfma_kernel<T>, T = 1 .. 4: two antenna counts per T, the second one whole tiles (48: the 16 idle load rows of a pass).
    # n_pts over {1, 3, kFT, kFT + 1, 2 kFT + 1}: several chunks inside one tile, a chunk that is exactly one tile, a tile that
    # begins in one chunk and ends in the next, fetch's fast path (2 kFT + 1, 3 at T = 1 never) beside its slow one
    _case("mfma", 9, 4096, 3, 4, tail=5, rot=True),
    _case("mfma", 16, 512, 17, 2),
    _case("mfma", 17, 512, 1, 3, tail=7, rot=True),
    _case("mfma", 32, 512, 4, 4),
    _case("mfma", 33, 256, 9, 4, tail=3, rot=True),
    _case("mfma", 48, 256, 5, 2),
    _case("mfma", 49, 256, 5, 4, tail=11, rot=True),
    _case("mfma", 64, 256, 3, 3),
    # xengine_kernel<A>: n_pts 1 and 3 (the one-spectrum tail of the kXU = 2 loop in every chunk of a group); the tiled F stage,
    # the wave-local one at 32 channels (part of a wave), the fused one at 4096 channels / 4 taps
    _case("vector", 3, 8192, 3, 4, tail=9, rot=True),
    _case("vector", 3, 32, 1, 2),
    _case("vector", 5, 8192, 1, 3, rot=True),
    _case("vector", 4, 4096, 3, 4, tail=5, path="fused"),
    _case("vector", 8, 8192, 1, 4, tail=77, rot=True),
    # xengine_kernel<A, true>: two antennas off the fused kernel, and four
    _case("autos", 2, 2048, 3, 4, tail=3, rot=True, autos=True),
    _case("autos", 4, 8192, 1, 2, autos=True),
    # a workspace small enough for three passes (a child process: FXC_WS_MB is read once), each with groups of its own
    _case("mfma", 9, 512, 3, 4, tail=1, rot=True, passes=True),
    _case("vector", 3, 8192, 1, 4, passes=True),
    # xengine_block_kernel (the developer library, FXC_XENGINE=block, a child process): two and three antenna blocks
    _case("block", 9, 2048, 1, 4),
    _case("block", 17, 1024, 3, 2, tail=3, rot=True),
]
BY_ID = {c.id: c for c in CASES}


# ---- the kernels' geometry, restated ---------------------------------------------------------------------------------------------
def tiles(case):
    """T of xengine_mfma_kernel<T>: antenna tiles of 16 (h_launch.h::FXC_XMFMA_DISPATCH)"""
    return min((case.n_ant + 15) // 16, 4)


def k_ft(t):
    """XMfmaGeo<T>::kFT, frames per LDS tile"""
    return 8 if t == 1 else 4


def mfma_lds_bytes(t):
    """XMfmaGeo<T>::kLdsBytes: two tiles of kFT frames x 16 T antennas, rows of 17 complex64 -- or the epilogue's 256 rows"""
    tile_cf = k_ft(t) * 16 * t * MFMA_PITCH
    return max(2 * tile_cf, 256 * MFMA_PITCH) * 8


def per_cu_bound(case):
    """workgroups of the case's X-engine kernel a CU holds at the most"""
    if case.kernel == "mfma":
        return LDS_PER_CU // mfma_lds_bytes(tiles(case))
    return ONE_WAVE_PER_CU


def cols(case):
    """workgroups a raw row takes: xengine_group's and autos_group's ``cols``"""
    if case.kernel == "mfma":
        return max(1, case.nchan // MFMA_COLUMN)
    if case.kernel == "autos":
        return max(1, -(-case.nchan // X_THREADS))
    gb = -(-case.n_ant // X_BLOCK)
    return max(1, case.nchan // X_THREADS) * (gb * (gb + 1) // 2 if case.kernel == "block" else 1)


def fused_unit(case):
    """h_launch.h::fused_unit: chunks a float32 raw row may hold"""
    return max(1, min(K_ROW_SPECTRA // max(1, case.n_pts), 64))


def groups_max(case, cu_count):
    return max(1, per_cu_bound(case) * cu_count // cols(case))


def group_size(case, nc, groups):
    """xengine_group / autos_group: chunks per raw row of a pass of nc chunks"""
    return max(1, min(fused_unit(case), -(-nc // groups)))


def cg_min(case, cu_count, nc):
    """the smallest group the device can choose for a pass of nc chunks: every workgroup the bound allows resident"""
    return group_size(case, nc, groups_max(case, cu_count))


def group_lengths(nc, cg):
    """chunks of every group of a pass: the kernels' ``c_end`` clamp"""
    return [min(cg, nc - c0) for c0 in range(0, nc, cg)]


def is_prime(n):
    return n >= 2 and all(n % d for d in range(2, int(n ** 0.5) + 1))


def next_prime(n):
    while not is_prime(n):
        n += 1
    return n


def pass_floor(case, cu_count):
    """chunks a pass needs for cg >= 3 and more than one group: past twice groups_max, and past fused_unit"""
    return max(2 * groups_max(case, cu_count) + 1, fused_unit(case) + 1)


def straddles(case, cg):
    """a tile of kFT frames holds frames of two chunks of a group of cg: a chunk boundary that is no tile boundary"""
    ft = k_ft(tiles(case))
    return any((j * case.n_pts) % ft for j in range(1, cg))


def fast_and_slow(case, cg):
    """(tiles of a full group that fetch takes at fixed strides, tiles it walks frame by frame): k_xmfma.h::fetch's condition"""
    ft, nfr = k_ft(tiles(case)), case.n_pts
    nf, q, i, fast, slow = nfr * cg, 0, 0, 0, 0
    while q < nf:
        if i + ft < nfr and q + ft <= nf:
            fast, q, i = fast + 1, q + ft, i + ft
        else:
            slow, q, i = slow + 1, q + ft, (i + ft) % nfr
    return fast, slow


# ---- passes: h_launch.h::fused_chunks_per_pass and h_run.h::autos_pass for chunks of one frame range ------------------------------
def n_prod(case):
    return case.n_ant * (case.n_ant - 1) // 2 + (case.n_ant if case.autos else 0)


def chunk_bytes(case):
    """(spectra, raw rows) of one chunk in the workspace"""
    return case.n_ant * case.n_pts * case.nchan * 8, n_prod(case) * case.nchan * 8


def chunks_per_pass(case, ws_bytes, n_chunks):
    return max(1, min(ws_bytes // sum(chunk_bytes(case)), n_chunks, 65535))


def r256(b):
    return (int(b) + 255) // 256 * 256


def workspace_bytes(case, cb):
    """what a call of passes of cb chunks carves (h_run.h::carve_ws with the fold's partial sums, h_launch.h::fold_part_bytes)"""
    spec, raw = chunk_bytes(case)
    row_len = n_prod(case) * case.nchan
    return r256(cb * spec) + r256(cb * raw) + max(1, min(32, (4 << 20) // row_len)) * row_len * 16


def pass_plan(case, cu_count):
    """(FXC_WS_MB, chunks per pass, chunks of the long call) of a passes case: the smallest workspace whose pass is a prime number
    of chunks above ``pass_floor`` and above the smallest such prime, which the third, last pass takes: passes of cb, cb and
    fewer chunks, each with cg >= 3 and a shorter last group"""
    last = next_prime(pass_floor(case, cu_count))
    per = sum(chunk_bytes(case))
    mb = max(1, (last * per) >> 20)
    while True:
        cb = (mb << 20) // per
        if cb > last and is_prime(cb):
            return mb, cb, 2 * cb + last
        mb += 1


def call_chunks(case, cu_count):
    """chunks of the case's second, long fx_accumulate call on a device of cu_count CUs"""
    if case.passes:
        return pass_plan(case, cu_count)[2]
    return next_prime(pass_floor(case, cu_count))


def pass_lengths(case, cu_count):
    """chunks of every pass of the long call"""
    n = call_chunks(case, cu_count)
    cb = pass_plan(case, cu_count)[1] if case.passes else chunks_per_pass(case, 12 << 30, n)
    return [min(cb, n - c0) for c0 in range(0, n, cb)]


def n_chunks(case, cu_count):
    return SHORT + call_chunks(case, cu_count)


def num_samp(case):
    return case.nchan * case.n_pts + case.tail


def input_bytes(case, cu_count):
    return n_chunks(case, cu_count) * case.n_ant * num_samp(case) * 8


# ---- input, tables, oracle -------------------------------------------------------------------------------------------------------
def pairs(n_ant):
    return [(a, b) for a in range(n_ant) for b in range(a + 1, n_ant)]


def delays(n_ant):
    return np.arange(n_ant) % 11


def seed(case):
    return 7000 + 100 * case.n_ant + case.n_pts + (50 if case.passes else 0)


@functools.lru_cache(maxsize=1)
def _samples(case, n):
    from effex_amd import synth
    # synth_iq's chunk c is samples c * num_samp .. of one stream: n chunks are one long chunk cut up (no loop over the chunks)
    ns = num_samp(case)
    x = synth.synth_iq(seed(case), 1, case.n_ant, n * ns, delays=delays(case.n_ant))[0]
    x = np.ascontiguousarray(x.reshape(case.n_ant, n, ns).transpose(1, 0, 2))
    x.setflags(write=False)
    return x


def samples(case, cu_count):
    """x [n_chunks, n_ant, num_samp] complex64 (read-only): synth_iq(seed, n_chunks, n_ant, num_samp, delays=delays(n_ant)) --
    every antenna its own delay, every chunk its own samples"""
    return _samples(case, n_chunks(case, cu_count))


def window(case):
    from effex_amd.window import design_window
    return design_window(case.ntaps, case.nchan)


def rot(case):
    import fx_oracle
    return fx_oracle.rot_table(case.nchan, BW, FREQ, TAU_ROT) if case.rot else None


def oracle_pairs(case):
    """the baselines the oracle computes: all of them, or -- from 49 antennas on -- those of antennas 0, 15, 16, 33 and n_ant - 1
    with every other antenna and every baseline inside the last pair of antenna tiles (antennas 48 ...): some of every pair of
    tiles that has any"""
    if case.n_ant < SUBSET_FROM:
        return pairs(case.n_ant)
    ends = {0, 15, 16, 33, case.n_ant - 1}
    first = 16 * (tiles(case) - 1)
    return [(a, b) for a, b in pairs(case.n_ant) if a in ends or b in ends or a >= first]


def integrate_pairs(x, nchan, win, which, rot_tab=None, autos=False):
    """fx_oracle.fx_integrate's arithmetic for the baselines ``which`` alone -> [len(which), nchan] complex128, and with ``autos``
    the antennas' fftshift(mean |spec_a|^2) [n_ant, nchan] float64 as well"""
    import fx_oracle
    n, n_ant, _ = x.shape
    ntaps = len(win) // nchan
    acc = np.zeros((len(which), nchan), np.complex128)
    pw = np.zeros((n_ant, nchan), np.float64)
    ia, ib = [a for a, _ in which], [b for _, b in which]
    n_spec = 0
    for c in range(n):
        specs = np.stack([fx_oracle.spectrometer_poly(x[c, a], ntaps, nchan, win) for a in range(n_ant)])
        n_spec += specs.shape[1]
        acc += (specs[ia] * np.conj(specs[ib])).sum(axis=1)
        if autos:
            pw += (np.abs(specs) ** 2).sum(axis=1)
    acc /= max(n_spec, 1)
    if rot_tab is not None:
        acc = acc * np.conj(rot_tab)
    acc = np.fft.fftshift(acc, axes=-1)
    return (acc, np.fft.fftshift(pw / max(n_spec, 1), axes=-1)) if autos else acc


@functools.lru_cache(maxsize=1)
def _oracle(case, n):
    import fx_oracle
    x = _samples(case, n)
    autos = None
    if case.n_ant < SUBSET_FROM and not case.autos:
        cross = fx_oracle.fx_integrate(x, case.nchan, window(case), rot=rot(case))
    elif case.autos:
        cross, autos = integrate_pairs(x, case.nchan, window(case), pairs(case.n_ant), rot(case), autos=True)
    else:
        cross = integrate_pairs(x, case.nchan, window(case), oracle_pairs(case), rot(case))
    return cross, autos


def oracle(case, cu_count):
    """(cross [len(oracle_pairs), nchan] complex128, autos [n_ant, nchan] float64 or None) over all chunks of both calls:
    fx_oracle.fx_integrate where it computes what the case needs -- every baseline, no autos -- and its arithmetic restated for a
    subset of the baselines or with the autos beside (``integrate_pairs``, held to fx_integrate by the host test)"""
    return _oracle(case, n_chunks(case, cu_count))


# ---- comparisons -----------------------------------------------------------------------------------------------------------------
def worst_row(got, ref):
    """(error, row) of the row with the largest max|got - ref| / max|ref| -- every row against its own largest value"""
    got, ref = np.asarray(got), np.asarray(ref)
    err = np.abs(got - ref).max(axis=-1) / np.abs(ref).max(axis=-1)
    if np.isnan(err).any():
        return float("nan"), int(np.argmax(np.isnan(err)))
    k = int(np.argmax(err))
    return float(err[k]), k


def rel_err(a, b):
    """The suite's metric: max|a - b| / max|b|."""
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


# ---- the device side, in the test's process or in a child ------------------------------------------------------------------------
def host(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def device_outputs(plan_mod, torch, xd, case, dev=False):
    """"integ": fx_accumulate(x[:SHORT]), fx_accumulate(x[SHORT:]), finalize SPECTRUM; "rows_mean": the float64 mean over the chunks
    of the plan's own fx_rows (cg = 1 always), summed on the device; "info": workspace bytes after the integration, CUs; "path" """
    out = {}
    with plan_mod.FxPlan(case.n_ant, case.nchan, case.ntaps, num_samp(case), window=window(case), autos=case.autos, dev=dev) as p:
        if case.rot:
            p.set_rot(rot(case))
        p.fx_accumulate(xd[:SHORT])
        p.fx_accumulate(xd[SHORT:])
        out["integ"] = host(p.finalize("SPECTRUM")).copy()
        info = p.info
        out["info"] = np.array([info["workspace_bytes"], info["cu_count"]])
        out["path"] = np.array([p.path])
        acc = None
        for c0 in range(0, xd.shape[0], 1024):
            part = p.fx_rows(xd[c0:c0 + 1024], "SPECTRUM").to(torch.complex128).sum(dim=0)
            acc = part if acc is None else acc + part
        out["rows_mean"] = host(acc / xd.shape[0])
    return out
