"""The fused 4096-channel kernel's exchanges through component planes (fx_fused4096.h "exchanges"), on the host: the
thread <-> branch map of phase 1, where every lane-addressed store lands and who reads it, the waves' private areas, and
the LDS banks of every read of a step -- through the header's own functions (tests/emul/emul_planes.cpp, g++), the
position of a hardware lane being wave * 64 + lane.  And, in the compiled library, that no lane-addressed store directly
follows a write of M0 (an SALU write of M0 needs a wait state before ds_write_addtid_b32 reads it)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from effex_amd import build as fx_build

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "effex_amd", "csrc")
THREADS = 512


@pytest.fixture(scope="module")
def planes(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("planes") / "libemul_planes.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", lib, os.path.join(HERE, "emul", "emul_planes.cpp")], check=True)
    return ctypes.CDLL(lib)


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def lane_fields(hw):
    """(antenna, k1, j0 or q1) of hardware thread hw in phases 2 and 3."""
    lane, wave = hw & 63, hw >> 6
    return lane >> 5, 2 * wave + ((lane >> 4) & 1), lane & 15


def test_branch_map_is_a_permutation_and_keeps_a_wave_on_64_consecutive_samples(planes):
    j = np.array([planes.planes_branch_of_thread(t) for t in range(256)])
    assert sorted(j) == list(range(256))
    assert all(planes.planes_thread_of_branch(int(j[t])) == t for t in range(256))
    # the map, written out
    for t in range(256):
        lane, wv = t & 63, t >> 6
        assert j[t] == ((lane >> 1) & 15) + 16 * ((lane & 1) | ((lane >> 5) << 1) | (wv << 2))
    # a wave-load of branch row r: the 64 lanes' samples are 64 consecutive ones (512 contiguous bytes)
    for wv in range(4):
        for r in range(16):
            offs = sorted(planes.planes_sample_offset(int(j[64 * wv + lane]), r) for lane in range(64))
            assert offs == list(range(offs[0], offs[0] + 64))


def test_exchange_1_hands_every_value_to_the_lane_that_reads_it(planes):
    rng = np.random.default_rng(1)
    src = rng.uniform(1.0, 2.0, size=(THREADS, 16, 2)).astype(np.float32)
    want = np.zeros_like(src)
    got = np.zeros_like(src)
    ndw = planes.planes_region_dwords()
    owner = np.zeros(ndw, np.int32)
    planes.planes_exchange1(vp(src), vp(want), vp(got), vp(owner))
    assert (owner != -2).all()                                   # no dword written twice
    assert (owner >= 0).sum() == THREADS * 32                    # 16 complex values a thread
    # a wave's stores: 64 dwords side by side in every row of its antenna's two planes
    for wave in range(8):
        d = np.flatnonzero((owner >= 64 * wave) & (owner < 64 * wave + 64))
        ant, wv = wave >> 2, wave & 3
        expect = sorted(ant * 9216 + c * 4608 + k1 * 288 + wv * 64 + lane for c in range(2) for k1 in range(16) for lane in range(64))
        assert d.tolist() == expect
        assert (owner[d] - 64 * wave == (d % 288) % 64).all()    # lane l at M0 + 4 l
    # phase 2, lane (antenna, k1, j0): value j1 is output k1 of the thread that owns branch set j0 + 16 j1
    for hw in range(THREADS):
        ant, k1, j0 = lane_fields(hw)
        for j1 in range(16):
            t = planes.planes_thread_of_branch(j0 + 16 * j1)
            assert (got[hw, j1] == want[ant * 256 + t, k1]).all(), (hw, j1)


def test_exchange_2_transposes_inside_16_lane_groups_and_stays_in_the_waves_own_rows(planes):
    rng = np.random.default_rng(2)
    src = rng.uniform(1.0, 2.0, size=(THREADS, 16, 2)).astype(np.float32)
    got = np.zeros_like(src)
    ndw = planes.planes_region_dwords()
    owner = np.zeros(ndw, np.int32)
    planes.planes_exchange2(vp(src), vp(got), vp(owner))
    assert (owner != -2).all() and (owner >= 0).sum() == THREADS * 32
    for hw in range(THREADS):
        q1 = hw & 15
        for j0 in range(16):
            assert (got[hw, j0] == src[(hw & ~15) + j0, q1]).all(), (hw, j0)
    # wave-private: wave w writes only rows 2 w, 2 w + 1 of the four planes -- the rows its own phase 2 read, nobody else's
    addr2 = np.zeros((THREADS, 16, 2), np.int32)
    planes.planes_read_addresses(2, vp(addr2))
    seen = set()
    for wave in range(8):
        d = np.flatnonzero((owner >> 6) == wave)
        rows = {(int(x) // 4608, (int(x) % 4608) // 288) for x in d}
        assert rows == {(p, 2 * wave + k) for p in range(4) for k in range(2)}
        assert not (seen & set(d.tolist()))
        seen |= set(d.tolist())
        read_rows = {(int(x) // 4608, (int(x) % 4608) // 288) for x in addr2[64 * wave:64 * wave + 64].ravel()}
        assert rows == read_rows


def banks_are_distinct(dwords_per_lane, width):
    """One lane group of one LDS instruction: dwords_per_lane[lane] = first dword; every lane touches `width` dwords."""
    banks = [(int(a) + k) % 64 for a in dwords_per_lane for k in range(width)]
    return len(set(banks)) == len(banks)


@pytest.mark.parametrize("which", [2, 3])
def test_exchange_reads_are_conflict_free(planes, which):
    """ds_read_b64: two groups of 32 lanes, 64 banks of 4 bytes."""
    addr = np.zeros((THREADS, 16, 2), np.int32)
    planes.planes_read_addresses(which, vp(addr))
    base = planes.planes_lds_offset(0) // 4
    assert planes.planes_lds_offset(0) % 256 == 0
    for wave in range(8):
        a = addr[64 * wave:64 * wave + 64]
        for u in range(8):
            for c in range(2):
                first = a[:, 2 * u, c]
                assert (a[:, 2 * u + 1, c] == first + 1).all() and (first % 2 == 0).all()      # one aligned 8-byte read
                for half in range(2):
                    assert banks_are_distinct(base + first[32 * half:32 * half + 32], 2), (which, wave, u, c, half)


def test_window_reads_are_conflict_free(planes):
    """ds_read_b128 of the window quads, column = hardware thread: four groups of 16 lanes."""
    quad = np.zeros((THREADS, 16), np.int32)
    planes.planes_window_reads(vp(quad))
    groups = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
    groups += [[lane + 32 for lane in g] for g in groups]
    base = planes.planes_lds_offset(1)
    assert base % 256 == 0 and base >= planes.planes_region_dwords() * 4
    for hw in range(THREADS):
        assert (quad[hw] == np.arange(16) * 256 + (hw & 255)).all()
    for wave in range(8):
        for r in range(16):
            for g in groups:
                assert banks_are_distinct([base // 4 + 4 * quad[64 * wave + lane, r] for lane in g], 4)


def test_the_store_bases_fit_the_16_bit_offset_of_m0(planes):
    """Base of a lane-addressed store = LDS address of the region + the wave's offset, behind at most the 20 480 bytes of
    static LDS of the variant with in-kernel DC removal; base + immediate + 4 * lane stays inside the region."""
    static_lds = 20480
    region = planes.planes_lds_offset(0)
    top1 = 36864 + 3 * 256                      # exchange 1: antenna 1, wave 3
    top2 = 7 * 2304                             # exchange 2: wave 7
    assert static_lds + region + max(top1, top2) < 65536
    assert top1 + 18432 + 15 * 1152 + 4 * 63 < planes.planes_region_dwords() * 4
    assert top2 + 57272 + 4 * 63 < planes.planes_region_dwords() * 4
    assert static_lds + planes.planes_lds_offset(3) + 64 <= 160 * 1024


needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not found")


@needs_hipcc
def test_no_lane_addressed_store_directly_after_a_write_of_m0(tmp_path):
    asm = tmp_path / "fxcorr.s"
    flags = [f for f in fx_build.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([fx_build.hipcc_path()] + flags + ["-S", "--cuda-device-only", "-o", str(asm), "fxcorr.hip"],
                   cwd=CSRC, check=True, stderr=subprocess.DEVNULL)
    text = open(asm).read()
    bodies = re.findall(r"^(\S*fx_fused4096_kernel\S*):(.*?)s_endpgm", text, re.S | re.M)
    assert len(bodies) == 5
    for name, body in bodies:
        ins = [line.strip() for line in body.split("\n") if line.startswith("\t") and line.strip() and line.strip()[0] not in ".;"]
        stores = [k for k, x in enumerate(ins) if x.startswith("ds_write_addtid_b32")]
        assert len(stores) == 4 * 64, (name, len(stores))                # 32 per exchange, two exchanges, four unrolled steps
        bad = [ins[k - 1] for k in stores if re.match(r"\S+\s+m0\b", ins[k - 1])]
        assert not bad, (name, bad[:4])
