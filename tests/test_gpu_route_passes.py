"""Every route of the one route ladder (h_run.h::fx_routes), both consumers, over several workspace passes, against the oracle.

fx_rows and fx_accumulate run the same pass loops, so a wrong pass offset would corrupt rows and integration alike -- and pass a
check of one against the other.  Each case therefore runs in a child process with the workspace target at 1 MiB (FXC_WS_MB is
read once per process), on the smallest shape of its route that has a pass boundary, takes at least three passes with a shorter
last one (the stream route, whose passes the grid bounds: two), and compares fx_rows and fx_accumulate + finalize with the float64 oracle: TOL_VIS of the largest magnitude of each
group of rows (cross, autos), TOL_CONT for the CONTINUUM values of two of the cases.

The passes are checked by the chunk arithmetic of the sizing functions (h_launch.h), which the workspace the call took confirms:
``cb`` chunks per pass = 1 MiB / (spec + raw bytes per chunk), and a fresh plan's first fx_rows leaves a workspace of
round256(cb spec) + round256(cb raw + lead).  ``raw`` is the route's raw rows per chunk (its frame splits at these sizes on the
MI355X's 256 CUs) times one row set; ``lead``: the fused kernel's leading-part rows, one per CU."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import fx_oracle
from effex_amd import synth
from effex_amd.window import design_window

pytestmark = pytest.mark.gpu

from tolerances import TOL_CONT, TOL_VIS

BW = 2.4e6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WS = 1 << 20


def case(name, n_ant, nchan, frames, n_chunks, path, spec, raw, ntaps=4, tail=5, lead=0, beside=0, autos=False, u8=False, cont=False):
    """spec, raw: bytes per chunk of the pass's spectra and raw rows; lead: bytes per CU of the leading-part rows after them; beside:
    bytes per chunk that the sizing counts and the route keeps outside the workspace"""
    return pytest.param(dict(n_ant=n_ant, nchan=nchan, ntaps=ntaps, num_samp=nchan * frames + tail, n_chunks=n_chunks, path=path,
                             spec=spec, raw=raw, lead=lead, beside=beside, autos=autos, u8=u8, cont=cont), id=name)


C = 8      # bytes of a complex64
CASES = [
    # the fused kernel, 2 antennas: one raw row per chunk, 32 chunks per pass
    case("fused-2", 2, 4096, 3, 70, "fused", 0, 4096 * C, lead=4096 * C, cont=True),
    case("fused-2-u8", 2, 4096, 3, 70, "fused", 0, 4096 * C, lead=4096 * C, u8=True),
    case("fused-2-autos", 2, 4096, 3, 23, "fused", 0, 3 * 4096 * C, lead=3 * 4096 * C, autos=True),            # rows of [3][4096]: 10
    # 3 and more antennas: spectra + one row set per chunk
    case("fused-route-3", 3, 4096, 2, 8, "tiled", 3 * 2 * 4096 * C, 3 * 4096 * C),                              # 3
    case("tiled-3", 3, 1024, 8, 11, "tiled", 3 * 8 * 1024 * C, 3 * 1024 * C, cont=True),                        # 4
    case("tiled-2", 2, 2048, 4, 150, "tiled", 0, 2048 * C),                                                     # 64
    case("two-pass-8192", 2, 8192, 2, 41, "tiled", 0, 2 * 8192 * C),                        # two runs of one frame: 8 (so 41 chunks, not 40)
    # two 4096-channel problems per chunk; their filtered samples (4 streams of 2 frames of 4096) lie in a buffer of their own: 3
    case("split-8192", 2, 8192, 2, 8, "tiled", 0, 2 * 4096 * C, ntaps=8, lead=4096 * C, beside=4 * 2 * 4096 * C),
    # the kernels per channel count (spec_wg_splits: a call this small takes runs of two frames): 20 runs of 40 frames, 6
    case("one-pass-1000", 2, 1000, 40, 23, "generic", 0, 20 * 1000 * C),
    # two passes of them: antenna 0's spectra + 3 runs of 6 frames, 2 (so 7 chunks, not 8: a shorter last pass)
    case("two-pass-6000", 2, 6000, 6, 7, "generic", 6 * 6000 * C, 3 * 6000 * C),
    # the any-shape one-pass kernel (x_geometry: runs of four frame groups at least, so one run): 5000 channels from bytes, 26
    case("one-pass-5000-u8", 2, 5000, 4, 60, "generic", 0, 5000 * C, u8=True),
    case("x-engine-1000", 3, 1000, 8, 11, "generic", 3 * 8 * 1000 * C, 3 * 1000 * C),                          # 4
    # ... and 58: a row of 464 bytes, 2259 chunks per pass
    case("any-shape-58", 2, 58, 40, 4523, "generic", 0, 58 * C),
    case("autos-3", 3, 512, 8, 19, "tiled", 3 * 8 * 512 * C, 6 * 512 * C, autos=True),                          # 8
    case("autos-2", 2, 1000, 8, 15, "generic", 2 * 8 * 1000 * C, 3 * 1000 * C, autos=True),                     # 6
    # the stream route's passes are bounded by 65 535 chunks (grid.y), not by the workspace: two passes
    case("stream", 2, 1, 8, 65540, "stream", 0, 0, tail=0),
]

CHILD = r'''
import json, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
from effex_amd.plan import FxPlan
c = json.loads(sys.argv[2])
x = torch.from_numpy(np.load(sys.argv[3])).cuda()
out = {}
with FxPlan(c["n_ant"], c["nchan"], c["ntaps"], c["num_samp"], autos=c["autos"]) as p:
    assert p.path == c["path"], (p.path, c["path"])
    rows = (lambda m: p.fx_rows_u8(x, m, %(bw)r, remove_dc=True)) if c["u8"] else (lambda m: p.fx_rows(x, m, %(bw)r))
    out["rows"] = rows("SPECTRUM").cpu().numpy()
    out["info"] = np.array([p.info["workspace_bytes"], p.info["cu_count"]])
    if c["cont"]:
        out["rows_c"] = rows("CONTINUUM").cpu().numpy()
    p.fx_accumulate_u8(x, remove_dc=True) if c["u8"] else p.fx_accumulate(x)
    out["integ"] = p.finalize("SPECTRUM", reset=False)
    out["integ_c"] = p.finalize("CONTINUUM", %(bw)r)
np.savez(sys.argv[4], **out)
''' % {"bw": BW}


def rel_err(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def samples(c):
    """the case's input as the plan takes it, and as the float64 oracle does"""
    if c["path"] == "stream":      # (65 540 chunks of 8 samples: cut from one long chunk)
        x = np.ascontiguousarray(synth.synth_iq(31, 1, 2, c["n_chunks"] * c["num_samp"])[0].reshape(2, c["n_chunks"], -1).transpose(1, 0, 2))
    else:
        x = synth.synth_iq(31, c["n_chunks"], c["n_ant"], c["num_samp"])
    if not c["u8"]:
        return x, x
    # the receivers' bytes: the same signal at a third of full scale, every stream with an offset of its own
    off = np.random.default_rng(31).uniform(-9, 9, size=(c["n_chunks"], c["n_ant"], 1, 2))
    q = np.stack([x.real, x.imag], axis=-1) * (42.0 / np.abs(x).max()) + 127.5 + off
    u8 = np.clip(np.rint(q), 0, 255).astype(np.uint8)
    z = fx_oracle.u8_to_complex(u8)
    for s in z.reshape(-1, z.shape[-1]):
        s[:] = fx_oracle.remove_dc(s)
    return u8, z


def oracle_rows(z, chunks, nchan, window, autos):
    """[chunk][cross rows, then auto rows][nchan], fft-shifted SPECTRUM values of the given chunks"""
    n_ant, ntaps = z.shape[1], len(window) // nchan
    pairs = [(a, b) for a in range(n_ant) for b in range(a + 1, n_ant)]
    out = np.zeros((len(chunks), len(pairs) + (n_ant if autos else 0), nchan), np.complex128)
    for i, ch in enumerate(chunks):
        specs = [fx_oracle.spectrometer_poly(z[ch, a], ntaps, nchan, window) for a in range(n_ant)]
        for r, (a, b) in enumerate(pairs):
            out[i, r] = np.fft.fftshift((specs[a] * np.conj(specs[b])).mean(axis=0))
        for a in range(n_ant if autos else 0):
            out[i, len(pairs) + a] = np.fft.fftshift((np.abs(specs[a]) ** 2).mean(axis=0))
    return out


@pytest.mark.parametrize("c", CASES)
def test_every_route_in_several_passes_matches_the_oracle(c):
    x, z = samples(c)
    with tempfile.TemporaryDirectory() as tmp:
        np.save(os.path.join(tmp, "x.npy"), x)
        proc = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps(c), os.path.join(tmp, "x.npy"), os.path.join(tmp, "r.npz")],
                              env=dict(os.environ, FXC_WS_MB="1"), capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
        got = {k: v for k, v in np.load(os.path.join(tmp, "r.npz")).items()}
    n, nchan, stream = c["n_chunks"], c["nchan"], c["path"] == "stream"
    ws, cu = (int(v) for v in got["info"])
    print("workspace %d bytes, %d CUs" % (ws, cu))

    # the oracle: every chunk -- the stream case's 65 540: the chunks at the ends of its two passes, and the mean of the rows
    chunks = [0, 1] + list(range(65534, n)) if stream else list(range(n))
    ref = oracle_rows(z, chunks, nchan, design_window(c["ntaps"], nchan), c["autos"])
    ref_i = got["rows"].astype(np.complex128).mean(axis=0) if stream else ref.mean(axis=0)
    nb = c["n_ant"] * (c["n_ant"] - 1) // 2
    groups = [slice(0, nb)] + ([slice(nb, None)] if c["autos"] else [])
    errs = {}
    for g in groups:
        errs["rows", g.start] = rel_err(got["rows"][chunks][:, g], ref[:, g])
        errs["integ", g.start] = rel_err(got["integ"][g], ref_i[g])
        if c["cont"]:
            errs["rows_c", g.start] = rel_err(got["rows_c"][:, g], ref[:, g].mean(axis=-1) / BW)
            errs["integ_c", g.start] = rel_err(got["integ_c"][g], ref_i[g].mean(axis=-1) / BW)
    print("errors:", errs)

    assert got["rows"].shape == (n, ref.shape[1], nchan) and got["integ"].shape == ref.shape[1:]
    for (what, _), err in errs.items():
        assert err < (TOL_CONT if what.endswith("_c") else TOL_VIS), (what, err)

    # the passes
    if stream:
        cb = 65535
        assert n > cb and n % cb
    else:
        cb = WS // (c["spec"] + c["raw"] + c["beside"])
        r256 = lambda b: (int(b) + 255) // 256 * 256
        assert ws == r256(cb * c["spec"]) + r256(cb * c["raw"] + c["lead"] * cu), (ws, cb)
        assert n > 2 * cb and n % cb, (n, cb)
