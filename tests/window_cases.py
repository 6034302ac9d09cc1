"""The window layouts of every route, driven with a rough window.

``design_window`` is smooth and nearly symmetric: neighbouring taps differ by 1e-4 of their value and ``h[n]`` is almost
``h[L - 1 - n]``, so a tap read from the neighbouring branch, a reversed tap order or a whole reversed window moves a result by
less than the parity bounds.  ``rough_window`` has independent standard-normal taps -- no symmetry, no smoothness, no zeros --
and exchanging any two of them moves the float64 oracle by at least ten times the ceilings (``test_window_taps_host.py`` proves
that for every case and mutation below; ``test_gpu_window_taps.py`` runs the cases on the device).

``CASES`` has one entry per distinct way the library stores or reads the window (h_build.h::plan_build, window_quads,
reversed_taps and the launchers of h_launch.h):

* quads ``f4[16][256]`` in LDS: the fused kernel (F + X, F only, byte ingest);
* quads of the tiled ring kernels (512 ... 4096 channels, every zero-padded width 1 ... 4) and of the wave-local kernels;
* 7 / 16 of the quads in LDS and the rest from L2: f8192_ring_kernel and its second-pass form;
* ``reversed_taps`` [tp][N]: pfb_prefilter_kernel<8 | 16 | 32> (8- and 16-byte accesses, streams side by side below 256
  channels) and pfb_split8192_kernel<4 | 8 | 16>, with the unit-tap quads / unit window of the kernels behind them;
* [ntaps][nchan] float: the 8192-channel pair kernel, the any-shape mixed-radix kernel (F + X, F only with two frames per
  slot, chirp-z rows, beyond LDS) and the generic FIR kernel;
* the kernels compiled per channel count: taps in LDS tables, or as quads from L2 in the lean builds (above 2048 channels, or
  with a prime factor of 17 ... 23), F + X, F only and second pass.

A new route, or a new way of holding taps, adds a line to ``CASES``.

Sizes: two chunks; ``num_samp = nchan * frames + extra``.  ``frames`` is just above ``ntaps`` -- a tap t meets data only from
frame t on, so fewer frames would hide the last taps from every check -- and behind a pre-filter or split pass it is
``2 * block + 3`` (block: the pass's register block of 8, 16 or 32 frames; 4 on the split's 4-tap form), which crosses a block
boundary of the pass; at most 67.
"""
import collections

import numpy as np

from effex_amd import synth

Case = collections.namedtuple("Case", "id n_ant nchan ntaps frames extra n_chunks entry env dev expect path")


def rough_window(ntaps, nchan):
    """[ntaps * nchan] float64, independent standard-normal taps: no symmetry, no smoothness, no zero taps."""
    return np.random.default_rng(1000003 * ntaps + nchan).standard_normal(ntaps * nchan)


def mutations(window, ntaps, nchan):
    """(name, wrong_window) pairs: the slips of a tap layout -- a neighbour's tap, a wrong end, a wrong order."""
    window = np.asarray(window, dtype=np.float64)
    assert window.shape == (ntaps * nchan,)
    branch = 7 * nchan // 16

    def swapped(i, j):
        w = window.copy()
        w[i], w[j] = window[j], window[i]
        return w

    mid = (ntaps // 2) * nchan + branch
    yield "mid_adjacent_swapped", swapped(mid, mid + 1)
    yield "last_two_swapped", swapped(ntaps * nchan - 1, ntaps * nchan - 2)
    yield "first_two_swapped", swapped(0, 1)
    if ntaps > 1:
        w = window.copy().reshape(ntaps, nchan)
        w[:, branch] = w[::-1, branch].copy()
        yield "one_branch_tap_order_reversed", w.reshape(-1)
    yield "whole_window_reversed", window[::-1].copy()


# ---- what plan.path and plan.info must show (fxc_plan_get_info), checked after the entry point ran -------------------------
def _tiled_lds(nchan, ring):
    return 2 * (nchan + nchan // 16) * 8 + 256 * 8 + (nchan * 16 if ring else 0)


def _fused():
    return {"path": "fused", "block": 512, "specialised": 0}


def _tiled(nchan, ring=True):          # the tiled workgroup kernels; ring: the frame ring in registers, window quads in LDS
    return {"path": "tiled", "block": nchan // 8, "lds_bytes": _tiled_lds(nchan, ring), "specialised": 0}


def _small(nchan):                     # the wave-local kernels
    return {"path": "tiled", "block": 256, "lds_bytes": nchan * 16 + 4 * 1088 * 8, "specialised": 0}


def _two_pass_8192():                  # f8192_ring_kernel and its second-pass form
    return {"path": "tiled", "block": 512, "specialised": 0}


def _generic(specialised=0):           # plans whose path is the generic one: the bits of the kernels built for the channel count
    return {"path": "generic", "specialised": specialised}


def _case(id, n_ant, nchan, ntaps, frames, extra, expect, entry="fx", env=None, dev=False, path=None):
    return Case(id, n_ant, nchan, ntaps, frames, extra, 2, entry, dict(env or {}), dev, expect, path)


_NO_RTC = {"FXC_RTC": "0"}

CASES = [
    # fused kernel: quads f4[16][256] in LDS
    _case("fused-4096x4", 2, 4096, 4, 7, 5, _fused()),
    _case("fused-f-only-4ant-4096x4", 4, 4096, 4, 6, 3, _fused()),
    _case("fused-bytes-4096x4", 2, 4096, 4, 7, 5, _fused(), entry="fx_u8"),
    # the F stage of a single stream at the headline shape: the F-only tiled ring kernel (a plan of one antenna reports the
    # generic path; fxc_channelize takes the tiled kernels wherever the shape has them)
    _case("channelize-4096x4", 1, 4096, 4, 7, 5, _generic(), entry="channelize"),
    # tiled ring kernels: every zero-padded quad width
    _case("ring-512x4", 2, 512, 4, 9, 5, _tiled(512)),
    _case("ring-1024x3", 2, 1024, 3, 7, 3, _tiled(1024)),
    _case("ring-2048x1", 2, 2048, 1, 5, 100, _tiled(2048)),
    _case("ring-4096x2", 2, 4096, 2, 6, 7, _tiled(4096)),
    _case("channelize-2048x4", 1, 2048, 4, 7, 9, _generic(), entry="channelize"),
    # wave-local kernels
    _case("wave-16x4", 2, 16, 4, 9, 3, _small(16)),
    _case("wave-64x3", 2, 64, 3, 7, 1, _small(64)),
    _case("wave-256x4", 2, 256, 4, 8, 7, _small(256)),
    _case("wave-128x1", 2, 128, 1, 5, 2, _small(128)),
    _case("channelize-32x4", 1, 32, 4, 9, 5, _generic(), entry="channelize"),
    # pre-filter pass: each register block at both ends of its tap range (block 8: an odd stream length takes 8-byte accesses,
    # an even one 16-byte accesses, two positions per thread)
    _case("pre8-1024x5", 2, 1024, 5, 19, 1, _tiled(1024)),
    _case("pre8-512x8-wide", 2, 512, 8, 19, 0, _tiled(512)),
    _case("pre16-2048x9", 2, 2048, 9, 35, 3, _tiled(2048)),
    _case("pre16-4096x16", 2, 4096, 16, 35, 0, _tiled(4096)),
    _case("pre32-512x17", 2, 512, 17, 67, 5, _tiled(512)),
    _case("pre32-2048x32", 2, 2048, 32, 67, 0, _tiled(2048)),
    # ... below 256 channels, streams side by side in a workgroup
    _case("pre16-side-by-side-64x16", 2, 64, 16, 35, 3, _small(64)),
    _case("pre32-side-by-side-16x32", 2, 16, 32, 67, 1, _small(16)),
    # 8192 channels in two passes: 7 / 16 of the quads in LDS, the rest from L2
    _case("two-pass-8192x4", 2, 8192, 4, 5, 1, _two_pass_8192()),
    _case("two-pass-8192x3", 2, 8192, 3, 6, 8191, _two_pass_8192()),
    # ... split into two 4096-channel problems: reversed taps [4 | 8 | 16][8192], unit-tap quads behind them
    _case("split8-8192x5", 2, 8192, 5, 19, 1, _tiled(8192, ring=False)),
    _case("split16-8192x9", 2, 8192, 9, 35, 3, _tiled(8192, ring=False)),
    _case("split16-8192x16", 2, 8192, 16, 35, 0, _tiled(8192, ring=False)),
    _case("split4-8192x4-wide", 2, 8192, 4, 11, 2, _tiled(8192, ring=False), env={"FXC_X8192": "0"}, dev=True),
    # ... the plain variant: pre-filter + the pair kernel on a unit window; 3 antennas and the F stage on the ring kernel; the pair
    # kernel on the window itself
    _case("plain-8192x17", 2, 8192, 17, 35, 5, _tiled(8192, ring=False)),
    _case("f-only-3ant-8192x4", 3, 8192, 4, 5, 3, _tiled(8192, ring=False)),
    _case("channelize-8192x4", 1, 8192, 4, 5, 1, _generic(), entry="channelize"),
    _case("channelize-pair-kernel-8192x4", 1, 8192, 4, 5, 1, _generic(), entry="channelize", env={"FXC_F8192": "0"}, dev=True),
    # kernels compiled per channel count (pre-built counts where one fits)
    _case("spec-1000x4", 2, 1000, 4, 9, 7, _generic(1)),
    _case("spec-250x2", 2, 250, 2, 7, 3, _generic(1)),
    _case("spec-lean-3000x4", 2, 3000, 4, 6, 1, _generic(1)),
    _case("spec-lean-prime17-1020x4", 2, 1020, 4, 7, 3, _generic(1)),
    _case("spec-f-only-channelize-3000x4", 1, 3000, 4, 6, 1, _generic(2), entry="channelize"),
    _case("spec-f-only-3ant-3000x4", 3, 3000, 4, 6, 1, _generic(2)),
    _case("spec-second-pass-5000x4", 2, 5000, 4, 6, 11, _generic(2 + 4)),
    # the any-shape mixed-radix kernel
    _case("mixed-1000x4", 2, 1000, 4, 9, 7, _generic(), env=_NO_RTC),
    _case("mixed-f-only-3ant-1000x4", 3, 1000, 4, 9, 7, _generic(), env=_NO_RTC),      # two consecutive frames share tap loads
    _case("mixed-chirpz-997x4", 2, 997, 4, 8, 3, _generic(), env=_NO_RTC),
    _case("mixed-beyond-lds-12000x4", 2, 12000, 4, 5, 7, _generic(), env=_NO_RTC),
    _case("mixed-7x32", 2, 7, 32, 40, 3, _generic(), env=_NO_RTC),
    # generic kernels: pfb_fir_kernel + the radix-2 transform
    _case("generic-256x4", 2, 256, 4, 8, 7, _generic(), path="generic"),
    _case("generic-2048x32", 2, 2048, 32, 35, 0, _generic(), path="generic"),
]


def num_samp(case):
    return case.nchan * case.frames + case.extra


def make_input(case):
    """-> (x, u8): ``x`` [n_chunks, n_ant, num_samp] is what the oracle takes -- the synthetic streams (complex64), or for a byte
    case the bytes converted and de-meaned in float64 as the reference does on the host; ``u8`` the bytes of a byte case, else
    None."""
    import fx_oracle
    n = num_samp(case)
    if case.entry == "fx_u8":
        u8 = np.random.default_rng(case.nchan + case.ntaps).integers(0, 256, size=(case.n_chunks, case.n_ant, n, 2), dtype=np.uint8)
        a = fx_oracle.u8_to_complex(u8)
        x = np.stack([np.stack([fx_oracle.remove_dc(a[c, s]) for s in range(case.n_ant)]) for c in range(case.n_chunks)])
        return x, u8
    x = synth.synth_iq(321 + case.nchan + case.ntaps, case.n_chunks, case.n_ant, n, delays=np.arange(case.n_ant) % 5)
    return x, None


def oracle(case, x, window):
    """What the device test compares with, from the float64 oracle: ``fx`` -> [n_chunks, n_baselines, nchan], chunk by chunk;
    ``channelize`` -> [n_streams, frames, nchan]."""
    import fx_oracle
    if case.entry == "channelize":
        flat = x.reshape(-1, x.shape[-1])
        return np.stack([fx_oracle.spectrometer_poly(s, case.ntaps, case.nchan, window) for s in flat])
    return np.stack([fx_oracle.fx_integrate(x[c:c + 1], case.nchan, window) for c in range(x.shape[0])])


def rel_err(a, b):
    """The suite's metric: max|a - b| / max|b|."""
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def checks(case, got, ref):
    """(label, error) of every comparison the device test makes of ``got`` with ``ref`` (both as ``oracle`` returns them): every
    chunk's row of baseline (0, 1) -- with 3 and more antennas also all baselines of chunk 0 -- or every stream's spectra."""
    if case.entry == "channelize":
        return [("stream %d" % s, rel_err(got[s], ref[s])) for s in range(ref.shape[0])]
    out = [("chunk %d (0,1)" % c, rel_err(got[c, 0], ref[c, 0])) for c in range(ref.shape[0])]
    if case.n_ant > 2:
        out.append(("chunk 0, all baselines", rel_err(got[0], ref[0])))
    return out
