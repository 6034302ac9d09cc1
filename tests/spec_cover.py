"""Which code of fx_spec.h a channel count runs, and the list of channel counts that between them run all of it.

A kernel compiled per channel count (fx_spec.h through hiprtc, h_rtc.h) is cut by its stage list and layout: which butterfly stands
in the first stage (inputs from the FIR ring), in a middle stage (twiddles, a trip through LDS) and in the last (the X multiply, the
natural-order store or the multiply with antenna 0's spectra), frames per step, the lean build, padding, planes, row groups, slots.
``features`` names these as tuples; ``tests/golden/spec_cover.json`` (written by tools/make_spec_cover.py) holds, per build variant, a
small set of channel counts whose features cover everything the measured table effex_amd/csrc/spec_tuned.h and a sample of the cost
model's choices use.  tests/test_spec_cover_host.py and tests/test_gpu_spec_cover.py run them.  A helper module, not a test.

Variants (fxc_spec_probe): 0 F + X of two antennas, 1 the same from bytes, 2 the F stage alone, 3 the second pass above 4096 channels.
"""
import ctypes
import json
import os
import re
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TUNED_PATH = os.path.join(ROOT, "effex_amd", "csrc", "spec_tuned.h")
COVER_PATH = os.path.join(HERE, "golden", "spec_cover.json")
EMUL_SRC = os.path.join(HERE, "emul", "emul_spec.cpp")

VARIANT_TAG = {0: "xf", 1: "xb", 2: "f", 3: "xm"}
TABLE_OF_VARIANT = {0: "kSpecTuned", 2: "kSpecTunedF", 3: "kSpecTunedXM"}
MAX_TABLE_STAGES = 8                 # SpecTuned::radix[8]
NOT_RECORDED = ("code_bytes", "vgprs", "resident", "source")      # what the compiler's version or the cache decides, not the search
_LIST_KEYS = ("stages", "groups", "pads")


def parse_tuned(path=TUNED_PATH):
    """-> {variant: [{"n", "u", "n_stages", "radix": [...]}, ...]} in the file's order, the {0, ...} sentinel dropped"""
    text = open(path).read()
    out = {}
    for variant, name in TABLE_OF_VARIANT.items():
        m = re.search(r"constexpr\s+SpecTuned\s+%s\[\]\s*=\s*\{(.*?)\n\};" % name, text, re.S)
        if m is None:
            raise ValueError("no table %s in %s" % (name, path))
        rows = []
        for n, u, ns, radix in re.findall(r"\{\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*\{([0-9,\s]*)\}\s*\}", m.group(1)):
            if int(n) == 0:
                continue
            rows.append({"n": int(n), "u": int(u), "n_stages": int(ns), "radix": [int(v) for v in radix.split(",") if v.strip()]})
        out[variant] = rows
    return out


def parse_report(text):
    rep = {}
    for kv in text.split():
        k, v = kv.split("=")
        rep[k] = [int(t) for t in v.split(",")] if k in _LIST_KEYS else (v if k == "source" else int(v))
    return rep


def probe_rc(nchan, ntaps, variant):
    """fxc_spec_probe for gfx950 (hiprtc compiles the library's own choice for this shape: no GPU needed) -> (rc, report dict or None)"""
    from effex_amd import _lib
    lib = _lib.load(dev=bool(os.environ.get("FXC_RTC_U")))      # (the knob that forces the frames per step exists in the developer library only)
    buf = ctypes.create_string_buffer(1024)
    rc = lib.fxc_spec_probe(nchan, ntaps, variant, b"gfx950", buf, len(buf))
    if rc != 0:
        return rc, None
    return 0, parse_report(buf.value.decode())


def probe(nchan, ntaps, variant):
    """the report as a dict (lists for stages / groups / pads), or None where the shape has no kernel of its own"""
    return probe_rc(nchan, ntaps, variant)[1]


def recorded(report):
    return {k: v for k, v in report.items() if k not in NOT_RECORDED}


def position(s, n_stages):
    return "only" if n_stages == 1 else ("first" if s == 0 else ("last" if s == n_stages - 1 else "mid"))


def static_features(variant, entry):
    """what a table entry says by itself: radix x position and frames per step"""
    ns = len(entry["radix"])
    return {(variant, "radix", r, position(s, ns)) for s, r in enumerate(entry["radix"])} | {(variant, "u", entry["u"])}


def features(variant, report):
    """The code paths of fx_spec.h this build takes, as a set of tuples (see the module's text).  "pad" is named for the stages that write
    a buffer (all but the last), "groups" and "twfull_covers" for the stages that read one (all but the first: the first has neither
    row groups nor twiddles)."""
    st, ns = report["stages"], len(report["stages"])
    n_rows = report["rows"] * report["frames_per_step"]
    f = {(variant, "radix", r, position(s, ns)) for s, r in enumerate(st)}
    f.add((variant, "u", report["frames_per_step"]))
    f.add((variant, "lean", report["lean"]))
    f.add((variant, "rows", report["rows"]))
    f.add((variant, "plane0", int(report["plane0"] != 0)))
    f.add((variant, "slots", 1 if report["slots"] == 1 else 2))
    for s in range(ns - 1):
        f.add((variant, "pad", position(s, ns), int(report["pads"][s] != 0)))
    for s in range(1, ns):
        g = report["groups"][s] if report["groups"][s] > 0 else n_rows
        f.add((variant, "groups", position(s, ns), 1 if g == 1 else 2))
        f.add((variant, "twfull_covers", st[s], int(report["twfull"] >= st[s])))
    nb0 = report["nchan"] // st[0]
    j0 = -(-nb0 // report["tpr"])
    f.add((variant, "tpr_partial", int(report["tpr"] * j0 != nb0)))
    return f


def load_cover(path=COVER_PATH):
    with open(path) as fh:
        return json.load(fh)


def cover_entries(cover=None):
    """[(variant, nchan, entry)] of the committed cover, in the file's order"""
    cover = cover or load_cover()
    return [(int(v), e["nchan"], e) for v in sorted(cover["cover"]) for e in cover["cover"][v]]


def as_tuples(lists):
    return {tuple(f) for f in lists}


# ---- the host emulation of one build (tests/emul/emul_spec.cpp compiled with the options the library hands hiprtc)

def emul_flags(report, u8=False, fonly=False, xm=False):
    st = report["stages"]
    join = lambda v: ",".join(str(t) for t in v)
    return ["-DFXM_N=%d" % report["nchan"], "-DFXM_T=%d" % report["ntaps"], "-DFXM_TPR=%d" % report["tpr"], "-DFXM_SLOTS=%d" % report["slots"],
            "-DFXM_NST=%d" % len(st), "-DFXM_RADICES=%s" % join(st), "-DFXM_U8=%d" % int(u8),
            "-DFXM_U=%d" % report["frames_per_step"], "-DFXM_FONLY=%d" % int(fonly or xm), "-DFXM_LEAN=%d" % report["lean"], "-DFXM_ROWS=%d" % report["rows"],
            "-DFXM_GROUPS=%s" % join(report["groups"]), "-DFXM_PADS=%s" % join(report["pads"]), "-DFXM_PLANE0=%d" % report["plane0"],
            "-DFXM_TWFULL=%d" % report["twfull"], "-DFXM_XM=%d" % int(xm)]


def build_emul(lib_path, flags):
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-pthread"] + list(flags) + ["-o", lib_path, EMUL_SRC], check=True)
    return ctypes.CDLL(lib_path)


def check_fx_emulation(tmp_path, nchan, ntaps, n_pts, wg_splits, u8, flags, tpr, slots, window=None):
    """The F + X build on the host: the sums over each slot's run of frames, added up over the slots, against the oracle's
    sum_i spec0[i] conj(spec1[i]) of the chunk, and the last slot's row against the sum over ITS run (1e-5 of the largest)."""
    import fx_oracle
    from effex_amd import synth
    from effex_amd.window import design_window
    lib = build_emul(str(tmp_path / "libemul_spec.so"), flags)
    assert lib.emul_spec_threads() == tpr * slots and lib.emul_spec_slots() == slots
    n_chunks, num_samp = 2, nchan * n_pts + min(3, nchan - 1)
    rng = np.random.default_rng(nchan * 7 + n_pts)
    if window is None:
        window = rng.standard_normal(ntaps * nchan) if nchan < 16 else design_window(ntaps, nchan)
    if u8:
        xb = rng.integers(0, 256, size=(n_chunks, 2, num_samp, 2), dtype=np.uint8)
        xb[:, 1, 2:] = xb[:, 0, :-2] // 2 + xb[:, 1, 2:] // 2
        dc = (rng.standard_normal((n_chunks, 2, 2)) * 0.1).astype(np.float32)            # conversion offsets [chunk][antenna] (re, im)
        x = (xb.astype(np.float32) / np.float32(127.5) + dc[:, :, None, :]).view(np.complex64)[..., 0]
        x_in, dc_in = xb, dc
    else:
        x = synth.synth_iq(nchan, n_chunks, 2, num_samp)
        x_in, dc_in = x, None
    tw = np.exp(2j * np.pi * np.arange(nchan) / nchan).astype(np.complex64)
    h32 = np.ascontiguousarray(window, dtype=np.float32)
    E = wg_splits * slots
    out = np.full((E, n_chunks, nchan), np.nan + 0j, dtype=np.complex64)
    lib.emul_spec_run.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_longlong] * 3 + [ctypes.c_int] * 2
    assert lib.emul_spec_run(x_in.ctypes.data, h32.ctypes.data, out.ctypes.data, tw.ctypes.data,
                             dc_in.ctypes.data if u8 else None, num_samp, n_pts, n_chunks, wg_splits, 1) == 0
    assert np.isfinite(out).all()
    got = out.astype(np.complex128).sum(axis=0)
    for c in range(n_chunks):
        s0 = fx_oracle.spectrometer_poly(x[c, 0], ntaps, nchan, window)
        s1 = fx_oracle.spectrometer_poly(x[c, 1], ntaps, nchan, window)
        ref = (s0 * np.conj(s1)).sum(axis=0)
        assert np.abs(got[c] - ref).max() <= 1e-5 * np.abs(ref).max(), (nchan, c)
    # a slot's row is the sum over ITS run of frames: slot e of E takes frames [e n_pts / E, (e + 1) n_pts / E)
    e = E - 1
    lo, hi = e * n_pts // E, (e + 1) * n_pts // E
    s0 = fx_oracle.spectrometer_poly(x[0, 0], ntaps, nchan, window)[lo:hi]
    s1 = fx_oracle.spectrometer_poly(x[0, 1], ntaps, nchan, window)[lo:hi]
    ref = (s0 * np.conj(s1)).sum(axis=0)
    assert np.abs(out[e, 0] - ref).max() <= 1e-5 * max(np.abs(ref).max(), 1e-30)


def check_f_emulation(tmp_path, nchan, ntaps, n_pts, wg_splits, n_streams, ant, flags, extra=None, window=None):
    """The F-only build on the host: every stream's spectra, natural bin order, in the antenna-interleaved layout
    ([chunk][frame][antenna][nchan]), against the oracle's spectrometer_poly (2e-6 of the largest)."""
    import fx_oracle
    from effex_amd import synth
    from effex_amd.window import design_window
    lib = build_emul(str(tmp_path / "libemul_spec_f.so"), flags)
    assert lib.emul_spec_fonly() == 1
    num_samp = nchan * n_pts + (min(2, nchan - 1) if extra is None else extra)
    rng = np.random.default_rng(nchan + n_streams)
    if window is None:
        window = rng.standard_normal(ntaps * nchan) if nchan < 16 else design_window(ntaps, nchan)
    x = synth.synth_iq(31 + nchan, n_streams, 1, num_samp)[:, 0]
    tw = np.exp(2j * np.pi * np.arange(nchan) / nchan).astype(np.complex64)
    h32 = np.ascontiguousarray(window, dtype=np.float32)
    assert n_streams % ant == 0
    out = np.full((n_streams // ant, n_pts, ant, nchan), np.nan + 0j, dtype=np.complex64)
    lib.emul_spec_run.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_longlong] * 3 + [ctypes.c_int] * 2
    assert lib.emul_spec_run(x.ctypes.data, h32.ctypes.data, out.ctypes.data, tw.ctypes.data, None, num_samp, n_pts, n_streams,
                             wg_splits, ant) == 0
    assert np.isfinite(out).all()
    for s_ in range(n_streams):
        ref = fx_oracle.spectrometer_poly(x[s_], ntaps, nchan, window)
        got = out[s_ // ant, :, s_ % ant, :]
        assert np.abs(got - ref).max() <= 2e-6 * np.abs(ref).max(), (nchan, s_)


def check_two_pass_emulation(tmp_path, nchan, ntaps, n_pts, wg_splits, f_shape, x_shape, n_chunks=3, extra=11):
    """Two passes on the host: antenna 0 of every chunk pair through the F-only build (streams two chunks apart), then antenna 1
    through the second-pass build whose last butterfly multiplies with antenna 0's spectra -- the sums over the slots' runs against
    the oracle's sum_i spec0[i] conj(spec1[i]) (1e-5 of the largest).  f_shape / x_shape: (flags, tpr, slots) of the two builds."""
    import fx_oracle
    from effex_amd import synth
    from effex_amd.window import design_window
    libs = []
    for tag, xm, shape in (("f", False, f_shape), ("x", True, x_shape)):
        flags, tpr, slots = shape
        assert "-DFXM_ROWS=1" in flags and slots == 1
        lib = build_emul(str(tmp_path / ("libemul_spec_%s.so" % tag)), flags)
        lib.emul_spec_run2.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_longlong] * 3 + [ctypes.c_int] * 2 + [ctypes.c_longlong, ctypes.c_void_p]
        assert lib.emul_spec_xm() == int(xm)
        libs.append(lib)
    f_lib, x_lib = libs
    num_samp = nchan * n_pts + extra
    window = design_window(ntaps, nchan)
    x = synth.synth_iq(nchan + 1, n_chunks, 2, num_samp)
    tw = np.exp(2j * np.pi * np.arange(nchan) / nchan).astype(np.complex64)
    h32 = np.ascontiguousarray(window, dtype=np.float32)
    spec0 = np.full((n_chunks, n_pts, nchan), np.nan + 0j, dtype=np.complex64)
    assert f_lib.emul_spec_run2(x.ctypes.data, h32.ctypes.data, spec0.ctypes.data, tw.ctypes.data, None, num_samp, n_pts, n_chunks,
                                wg_splits, 1, 2 * num_samp, None) == 0
    for c in range(n_chunks):
        ref = fx_oracle.spectrometer_poly(x[c, 0], ntaps, nchan, window)
        assert np.abs(spec0[c] - ref).max() <= 1e-5 * np.abs(ref).max()
    out = np.full((wg_splits, n_chunks, nchan), np.nan + 0j, dtype=np.complex64)
    ant1 = x.reshape(-1)[num_samp:]
    assert x_lib.emul_spec_run2(ant1.ctypes.data, h32.ctypes.data, out.ctypes.data, tw.ctypes.data, None, num_samp, n_pts, n_chunks,
                                wg_splits, 1, 2 * num_samp, spec0.ctypes.data) == 0
    assert np.isfinite(out).all()
    got = out.astype(np.complex128).sum(axis=0)
    for c in range(n_chunks):
        s0 = fx_oracle.spectrometer_poly(x[c, 0], ntaps, nchan, window)
        s1 = fx_oracle.spectrometer_poly(x[c, 1], ntaps, nchan, window)
        ref = (s0 * np.conj(s1)).sum(axis=0)
        assert np.abs(got[c] - ref).max() <= 1e-5 * np.abs(ref).max(), (nchan, c)
