"""The single-pulse search on the GPU (include/fxcorr.h fxc_boxcar_search, FxPlan.boxcar_search) against the numpy restatement of
its definition (boxcar_ref.py).  The three maps must EQUAL the restatement's bits on host and on device input, and the statistics
its float64 values: every step is a single IEEE operation in a fixed order, so there is nothing to tolerate.  Bits: no output
depends on the tiles, on host against device input, on the alignment of a device tensor or on the workspace target; the call
leaves its input and a delay track's counter alone."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import boxcar_ref as ref
import dedisperse_ref
from boxcar_ref import bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 4096           # kBoxT of effex_amd/csrc/k_boxcar.h: the starts of a filter tile
NCHAN = 64         # the plans' channel count: the search does not read it


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def plan_mod(torch):
    from effex_amd import plan
    return plan


@pytest.fixture(scope="module")
def plan(plan_mod):
    with plan_mod.FxPlan(2, NCHAN, 4, NCHAN * 8) as p:
        yield p


def same(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(bits(got), bits(want))


def same_stats(got, want):
    return got.shape == want.shape and got.dtype == np.float64 and np.array_equal(got, want, equal_nan=True)


def check(plan, torch, x, widths, block, clip=3.0, clip_iters=2, want=None):
    """host and device input against the restatement -> the restatement's result"""
    if want is None:
        want = ref.search(x, widths, block, clip, clip_iters)
    host = plan.boxcar_search(x, widths, block, clip, clip_iters, return_stats=True)
    assert all(isinstance(a, np.ndarray) for a in host)
    dev = plan.boxcar_search(torch.from_numpy(x).cuda(), widths, block, clip, clip_iters, return_stats=True)
    assert all(a.is_cuda for a in dev[:3]) and isinstance(dev[3], np.ndarray)
    assert dev[0].dtype == torch.float32 and dev[1].dtype == torch.int32 and dev[2].dtype == torch.int32
    for kind, got in (("host", host), ("device", [a.cpu().numpy() for a in dev[:3]] + [dev[3]])):
        for name, g, w in zip(("snr", "width", "time"), got, want):
            differ = int((bits(g) != bits(w)).sum()) if g.shape == w.shape else -1
            assert same(g, w), (kind, name, x.shape, widths, block, clip, clip_iters, "cells that differ", differ)
        assert same_stats(got[3], want[3]), (kind, "stats", x.shape, clip, clip_iters, got[3], want[3])
    return want


# -- shapes -------------------------------------------------------------------------------------------------------------------------
# rows x n_t: one sample (degenerate); two; one short of a segment; one past it; one start past a tile; a halo longer than what is
# left of the row; 256 * 256 + 300 samples: the second level of the tree with a partial segment and a partial group
SHAPES = [(3, 1), (2, 2), (5, 255), (4, 257), (2, T + 1), (2, T + 4096), (3, 65836)]
WIDTHS = [(0, 0), (3, 3), (0, 3), (12, 12), (5, 12), (0, 12)]


def blocks_of(n_t):
    return (1, 37, 256, T + 1, n_t + 5)


@pytest.mark.parametrize("n_rows,n_t", SHAPES)
def test_outputs_equal_the_restatement(plan, torch, n_rows, n_t):
    x = ref.loud_rows(np.random.default_rng(n_rows * 100003 + n_t), n_rows, n_t)
    turn = 0
    for widths in WIDTHS:
        if (1 << widths[0]) > n_t:
            continue                       # no start: an argument error, test_boxcar_argument_checks
        for block in blocks_of(n_t):
            clip_iters = (0, 1, 4)[turn % 3]
            turn += 1
            want = check(plan, torch, x, widths, block, 3.0, clip_iters)
            assert want[0].shape == (n_rows, -(-(n_t - (1 << widths[0]) + 1) // block))
    assert turn >= 5
    if n_t == 1:
        want = ref.search(x, (0, 0), 1)
        assert (bits(want[0]) == 0).all() and (want[3][:, 1] == 0).all() and (want[3][:, 2] == 1).all()


@pytest.mark.parametrize("n_rows,n_t", [(5, 255), (2, T + 4096)])
def test_every_node_of_the_tree(plan, torch, n_rows, n_t):
    """block = 1 with a single width is the whole matched-filtered series of that width"""
    x = ref.loud_rows(np.random.default_rng(n_t), n_rows, n_t)
    for j in range(13):
        if (1 << j) > n_t:
            break
        want = check(plan, torch, x, (j, j), 1, 3.0, 2)
        assert want[0].shape == (n_rows, n_t - (1 << j) + 1) and (want[1] == j).all()


def test_the_clipping_rounds_differ_and_clip_0_has_none(plan, torch):
    x = ref.loud_rows(np.random.default_rng(21), 4, 1000)
    seen = []
    for clip, clip_iters in ((3.0, 0), (3.0, 1), (3.0, 2), (3.0, 4), (0.0, 3), (2.0, 2), (1e-6, 2)):
        want = check(plan, torch, x, (0, 8), 64, clip, clip_iters)
        seen.append(want[3][:, 1])
    assert (seen[1] < seen[0]).all() and (seen[2] < seen[1]).all()      # the spikes leave, the std falls
    assert np.array_equal(seen[4], seen[0])                             # clip = 0: no round after round 0
    assert (seen[6] == 0).all()                                         # a round that counts fewer than 2 samples: degenerate


def test_ties_and_constant_rows(plan, torch):
    """a row of small integers with two equal spikes and a plateau whose S/N at width 4 equals the spikes' at width 1: the
    narrowest width and the earliest start win; a constant row is degenerate"""
    for n_t in (704, T + 300):
        x = np.stack([ref.tie_row(n_t), np.full(n_t, 2.5, np.float32), ref.loud_rows(np.random.default_rng(n_t), 1, n_t)[0]])
        for widths in ((0, 5), (0, 12), (2, 2)):
            for block in (1, 37, 256, T + 1, n_t):
                for clip_iters in (0, 2):
                    snr, width, time, stats = check(plan, torch, x, widths, block, 3.0, clip_iters)
                    assert (bits(snr[1]) == 0).all() and (width[1] == widths[0]).all() and stats[1, 1] == 0 and stats[1, 0] == 2.5
                    assert np.array_equal(time[1], np.arange(snr.shape[1]) * min(block, n_t))
                    assert stats[0, 0] == 0.0
                    if widths[0] == 0 and block == 37:
                        assert (width[0, 2], time[0, 2]) == (0, 77)      # not width 4 at 87, not the spike at 82


# -- bits -------------------------------------------------------------------------------------------------------------------------
def test_a_device_tensor_off_16_bytes(plan, torch):
    n_rows, n_t = 3, 1001              # rows 4004 bytes apart: every alignment of a row modulo 16
    x = ref.loud_rows(np.random.default_rng(8), n_rows, n_t)
    want = ref.search(x, (0, 8), 37)
    flat = torch.empty(x.size + 1, dtype=torch.float32, device="cuda")
    view = flat[1:].view(x.shape)
    view.copy_(torch.from_numpy(x))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 and flat.data_ptr() % 16 == 0
    got = plan.boxcar_search(view, (0, 8), 37)
    assert all(same(g.cpu().numpy(), w) for g, w in zip(got, want))
    outs = []
    for dtype, fill in ((torch.float32, -7.0), (torch.int32, -7), (torch.int32, -7)):
        outs.append(torch.full((want[0].size + 1,), fill, dtype=dtype, device="cuda")[1:].view(want[0].shape))
        assert outs[-1].data_ptr() % 16 == 4
    res = plan.boxcar_search(view, (0, 8), 37, out=outs)
    assert all(r is o for r, o in zip(res, outs)) and all(same(o.cpu().numpy(), w) for o, w in zip(outs, want))
    host_out = [np.zeros(want[0].shape, np.float32), np.zeros(want[0].shape, np.int32), np.zeros(want[0].shape, np.int32)]
    plan.boxcar_search(x, (0, 8), 37, out=host_out)
    assert all(same(o, w) for o, w in zip(host_out, want))


def test_outputs_do_not_depend_on_the_slabs(plan, torch):
    """A workspace target of 1 MiB (FXC_WS_MB is read once per process: a child) against the default here: 12 host rows of 65 836
    samples go through in slabs of 3, two rows of 300 000 samples -- each larger than the target -- one at a time; with block = T + 1
    the partial bests share the workspace.  The same bits, and the restatement's"""
    rng = np.random.default_rng(9)
    cases = {"a": (ref.loud_rows(rng, 12, 65836), (0, 8), 64), "b": (ref.loud_rows(rng, 2, 300000), (0, 12), T + 1)}
    want = {k: ref.search(x, w, b) for k, (x, w, b) in cases.items()}
    code = ("import numpy as np, torch, sys; sys.path.insert(0, %r); from effex_amd import plan\n"
            "d = np.load(sys.argv[1]); out = {}\n"
            "with plan.FxPlan(2, %d, 4, %d) as p:\n"
            "    for k, w, b in (('a', (0, 8), 64), ('b', (0, 12), %d)):\n"
            "        h = p.boxcar_search(d[k], w, b, return_stats=True)\n"
            "        g = p.boxcar_search(torch.from_numpy(d[k]).cuda(), w, b, return_stats=True)\n"
            "        for i in range(4):\n"
            "            out['h%%s%%d' %% (k, i)] = h[i]\n"
            "            out['d%%s%%d' %% (k, i)] = g[i].cpu().numpy() if i < 3 else g[i]\n"
            "np.savez(sys.argv[2], **out)\n" % (ROOT, NCHAN, NCHAN * 8, T + 1))
    with tempfile.TemporaryDirectory() as tmp:
        np.savez(os.path.join(tmp, "in.npz"), **{k: c[0] for k, c in cases.items()})
        res = os.path.join(tmp, "one.npz")
        subprocess.run([sys.executable, "-c", code, os.path.join(tmp, "in.npz"), res], check=True, env=dict(os.environ, FXC_WS_MB="1"),
                       timeout=600)
        small = dict(np.load(res))
    for k, (x, w, b) in cases.items():
        for i in range(3):
            assert same(small["h%s%d" % (k, i)], want[k][i]) and same(small["d%s%d" % (k, i)], want[k][i]), (k, i)
        assert same_stats(small["h%s3" % k], want[k][3]) and same_stats(small["d%s3" % k], want[k][3])
        check(plan, torch, x, w, b, want=want[k])


def test_inputs_and_the_track_are_left_alone(plan_mod, torch):
    x = ref.loud_rows(np.random.default_rng(10), 2 * 3, 900).reshape(2, 3, 900)
    keep = x.copy()
    want = ref.search(x, (0, 8), 64)
    assert want[0].shape == (2, 3, 15)
    with plan_mod.FxPlan(4, NCHAN, 4, NCHAN * 8) as plan:
        plan.set_delay_track(np.linspace(0.0, 1e-7, 4), np.zeros(4), 2.4e6, 1.4204e9)
        plan.track_seek(5)
        dev = torch.from_numpy(x).cuda()
        assert all(same(g, w) for g, w in zip(plan.boxcar_search(x), want))                      # the defaults
        assert all(same(g.cpu().numpy(), w) for g, w in zip(plan.boxcar_search(dev), want))
        assert plan.track_chunk == 5
        assert np.array_equal(bits(dev.cpu().numpy()), bits(keep)) and np.array_equal(bits(x), bits(keep))
        one = plan.boxcar_search(x[1, 2])                                                       # one axis: one row
        assert all(same(g, w[1, 2]) for g, w in zip(one, want))


# -- closure on the device ----------------------------------------------------------------------------------------------------------
def test_the_wide_pulse_from_power_to_candidates(plan_mod, torch):
    """the wide-pulse case's power through dedisperse on a CUDA tensor, boxcar_search on its result without leaving the device:
    sift_pulses' first candidate is the injected (series 1, trial 4, t 300, width 8), and the map equals the restatement applied to
    the library's own dedisperse output"""
    power, shifts, _ = ref.wide_pulse_case(0)
    with plan_mod.FxPlan(2, dedisperse_ref.WIDE_NCHAN, 4, dedisperse_ref.WIDE_NCHAN * 8) as plan:
        ts = plan.dedisperse(torch.from_numpy(power).cuda(), shifts)
        assert ts.is_cuda and tuple(ts.shape) == (2, 9, 637)
        snr, width, time = plan.boxcar_search(ts, widths=(0, 5), block=1, clip=3.0, clip_iters=2)
        assert snr.is_cuda and width.is_cuda and time.is_cuda and tuple(snr.shape) == (2, 9, 637)
        cands = plan_mod.sift_pulses(snr, width, time, threshold=6.0)
        print(cands[:3])
        first = cands[0]
        assert (first["series"], first["dm_index"], first["time"], first["width"]) == (1, 4, 300, 8)
        want = ref.search(ts.cpu().numpy(), (0, 5), 1, 3.0, 2)
        assert all(same(g.cpu().numpy(), w) for g, w in zip((snr, width, time), want))
        coarse = plan.boxcar_search(ts)                          # the defaults: widths (0, 8), blocks of 64
        first = plan_mod.sift_pulses(*coarse)[0]
        assert (first["series"], first["dm_index"], first["time"], first["width"]) == (1, 4, 300, 8)


# -- arguments ----------------------------------------------------------------------------------------------------------------------
def test_boxcar_argument_checks(plan, torch):
    from effex_amd import _lib
    x = ref.loud_rows(np.random.default_rng(13), 3, 100)

    def call(ptr, n_rows=3, n_t=100, kind=_lib.FXC_MEM_HOST, j_lo=0, j_hi=5, block=10, clip=3.0, clip_iters=2, plan_h=True, outs=(1, 1, 1)):
        o = [np.full((3, 10), -7.0, np.float32), np.full((3, 10), -7, np.int32), np.full((3, 10), -7, np.int32)]
        stats = np.full((3, 3), -7.0)
        rc = plan._lib.fxc_boxcar_search(plan._h if plan_h else None, ptr, n_rows, n_t, kind, j_lo, j_hi, block, clip, clip_iters,
                                         *[a.ctypes.data if on else None for a, on in zip(o, outs)], stats.ctypes.data)
        if rc != 0:
            assert all((a == -7).all() for a in o) and (stats == -7).all(), "outputs written on an error"
        return rc

    ptr = x.ctypes.data
    for change in (dict(ptr=None), dict(plan_h=False), dict(outs=(0, 1, 1)), dict(outs=(1, 0, 1)), dict(outs=(1, 1, 0)), dict(n_rows=0),
                   dict(n_rows=-1), dict(n_t=0), dict(n_t=-5), dict(block=0), dict(block=-3), dict(j_lo=-1), dict(j_hi=13), dict(j_lo=6),
                   dict(j_lo=7, j_hi=8), dict(clip=-1.0), dict(clip=float("nan")), dict(clip_iters=-1), dict(clip_iters=5), dict(kind=7),
                   dict(kind=_lib.FXC_MEM_DEVICE_TO_PINNED)):
        args = dict(ptr=ptr)
        args.update(change)
        rc = call(**args)
        assert rc == _lib.FXC_ERR_ARG, change
        if "plan_h" not in change:
            with pytest.raises(ValueError):
                _lib.check(rc, plan._h)
    assert call(ptr) == 0 and call(ptr, j_lo=6, j_hi=6, block=4) == 0            # 2^6 <= 100 < 2^7
    # n_t >= 2^31 through the arguments alone: nothing that large is allocated or read
    for n_t in (1 << 31, 1 << 40):
        rc = call(ptr, n_t=n_t)
        assert rc == _lib.FXC_ERR_UNSUPPORTED
        with pytest.raises(NotImplementedError):
            _lib.check(rc, plan._h)
    assert call(ptr, n_t=1 << 31, clip=-1.0) == _lib.FXC_ERR_ARG
    # the Python exceptions
    dev = torch.from_numpy(x).cuda()
    shape = (3, 10)
    good = [np.zeros(shape, np.float32), np.zeros(shape, np.int32), np.zeros(shape, np.int32)]
    for bad in (dict(widths=(-1, 3)), dict(widths=(0, 13)), dict(widths=(4, 3)), dict(widths=(7, 8)), dict(widths=3), dict(block=0),
                dict(clip=-1.0), dict(clip_iters=5), dict(out=good[:2]), dict(out=[good[0], good[1].astype(np.float32), good[2]]),
                dict(out=[good[0][:, :9], good[1], good[2]]), dict(out=[torch.from_numpy(a).cuda() for a in good])):
        args = dict(widths=(0, 5), block=10)
        args.update(bad)
        with pytest.raises(ValueError):
            plan.boxcar_search(x, **args)
    with pytest.raises(ValueError):
        plan.boxcar_search(dev, (0, 5), 10, out=good)                              # mixed host and device memory
    for bad_ts in (x.astype(np.float64), x.reshape(1, 1, 3, 100), x[:, :0], dev.double(), torch.from_numpy(x), x.tolist()):
        with pytest.raises(ValueError):
            plan.boxcar_search(bad_ts, (0, 5), 10)
    assert plan.boxcar_search(x, (0, 5), 10, out=good)[0] is good[0]
