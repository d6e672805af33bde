"""The bandit rollout's packed y cache (csrc/dpt_ycache.h) on the host: the 24-bit fixed-point
element format, the 12-B lane packing and the row layout.  CPU only: the header is plain C++
apart from its device fast paths, compiled here with the host compiler into a tiny shared object.

The folded weights (derive_l0_kernel's second set) live in device memory only and the C ABI has
no accessor for derived weights; adding one for this test alone is not cheap, so the fold is
covered by the oracle parity of tests/test_gpu_ycache_packed.py (every logit depends on it)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "decision-pretrained-transformer_amd", "csrc")
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")

SRC = r"""
#include "dpt_ycache.h"
using namespace dpt;
extern "C" {
int yq_quant_c(float y) { return yq_quant(y); }
// n (a multiple of 4) values: quantise, pack four to a lane, unpack, back to the value
void yq_roundtrip_c(const float* in, float* out, int* q8, int n) {
    for (int i = 0; i < n; i += 4) {
        const YqLane p = yq_pack(yq_quant(in[i]), yq_quant(in[i + 1]), yq_quant(in[i + 2]), yq_quant(in[i + 3]));
        out[i] = yq_value<0>(p); out[i + 1] = yq_value<1>(p); out[i + 2] = yq_value<2>(p); out[i + 3] = yq_value<3>(p);
        q8[i] = yq_unpack_q8<0>(p); q8[i + 1] = yq_unpack_q8<1>(p); q8[i + 2] = yq_unpack_q8<2>(p); q8[i + 3] = yq_unpack_q8<3>(p);
    }
}
long long yq_row_offset_c(int p, int t, int tile, int max_pos) { return yq_row_offset(p, t, tile, max_pos); }
}
"""

BOUND = 2.0 ** -21


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("ycache")
    src = d / "yq.cpp"
    src.write_text(SRC)
    so = d / "libyq.so"
    subprocess.run([CXX, "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + CSRC, str(src), "-o", str(so)], check=True)
    L = ctypes.CDLL(str(so))
    L.yq_quant_c.restype = ctypes.c_int
    L.yq_quant_c.argtypes = [ctypes.c_float]
    L.yq_row_offset_c.restype = ctypes.c_longlong
    L.yq_row_offset_c.argtypes = [ctypes.c_int] * 4
    return L


def roundtrip(L, x):
    x = np.ascontiguousarray(x, np.float32)
    n = (len(x) + 3) // 4 * 4
    xin = np.zeros(n, np.float32)
    xin[: len(x)] = x
    out = np.empty(n, np.float32)
    q8 = np.empty(n, np.int32)
    fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)
    L.yq_roundtrip_c(xin.ctypes.data_as(fp), out.ctypes.data_as(fp), q8.ctypes.data_as(ip), n)
    return out[: len(x)], q8[: len(x)]


def test_roundtrip_error_within_half_step(lib):
    """|value(pack(quant(x))) - x| <= 2^-21 on a dense grid over the LayerNorm range, its ends
    +-sqrt(31), +-0 and values just inside each side of rounding boundaries; every lane slot."""
    grid = np.linspace(-5.6, 5.6, 400001).astype(np.float32)
    ends = np.array([np.sqrt(31.0), -np.sqrt(31.0), 0.0, -0.0], np.float32)
    # rounding boundaries (k + 1/2) 2^-20 and the floats next to them on both sides
    k = np.array([0, 1, 2, 255, 256, 257, 65535, 65536, 1 << 20, (1 << 22) + 12345, 5 * (1 << 20) + 7], np.float64)
    mid = ((k + 0.5) * 2.0 ** -20).astype(np.float32)
    below, above = np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(10))
    edges = np.concatenate([below, mid, above, -below, -mid, -above]).astype(np.float32)
    for shift in range(4):  # every value passes through every one of the lane's four slots
        x = np.concatenate([np.zeros(shift, np.float32), grid, ends, edges])
        got, q8 = roundtrip(lib, x)
        err = np.abs(got.astype(np.float64) - x.astype(np.float64))
        assert err.max() <= BOUND, (shift, err.max(), x[err.argmax()])
        assert (q8 & 0xff == 0).all()  # q << 8: the float conversion is exact (24 significant bits)
        assert np.array_equal(got, (q8.astype(np.float64) * 2.0 ** -28).astype(np.float32))
    z, _ = roundtrip(lib, np.array([0.0, -0.0], np.float32))
    assert (z == 0).all()


def test_rounding_is_to_nearest(lib):
    assert lib.yq_quant_c(0.0) == 0 and lib.yq_quant_c(-0.0) == 0
    step = 2.0 ** -20
    for k in (0, 1, 7, 12345, 5 << 20):
        assert lib.yq_quant_c(np.float32(k * step)) == k
        assert lib.yq_quant_c(np.float32(-k * step)) == -k
        assert lib.yq_quant_c(np.float32((k + 0.25) * step)) == k
        assert lib.yq_quant_c(np.float32((k + 0.75) * step)) == k + 1
        assert lib.yq_quant_c(np.float32(-(k + 0.75) * step)) == -(k + 1)


def test_saturates_without_wrapping(lib):
    top = (1 << 23) - 1
    for v in (8.0, 8.5, 100.0, 3e38, np.inf):
        assert lib.yq_quant_c(np.float32(v)) == top
        assert lib.yq_quant_c(np.float32(-v)) == -top
    assert lib.yq_quant_c(np.nextafter(np.float32(8.0), np.float32(0))) == top
    x = np.array([8.0, -8.0, 1e9, -1e9, np.inf, -np.inf, 7.9999995, -7.9999995], np.float32)
    got, q8 = roundtrip(lib, x)
    assert np.array_equal(q8 >> 8, np.where(x > 0, top, -top))
    assert np.array_equal(np.sign(got), np.sign(x))  # clamped, not wrapped to the other sign
    assert np.allclose(np.abs(got), top * 2.0 ** -20, rtol=0, atol=0)


@pytest.mark.parametrize("tile", [8, 16])
@pytest.mark.parametrize("H", [1, 2, 7, 8, 9, 17, 20, 64, 70, 130, 500])
def test_row_layout_is_disjoint_and_inside_the_slot(lib, tile, H):
    """Rows of a tile are disjoint 96-B ranges inside H x tile x 96 B (the fp32 slot is H x tile x
    128 B); in whole 8-position groups a task's 8 rows are one 768-B run aligned to 128 B."""
    off = np.array([[lib.yq_row_offset_c(p, t, tile, H) for t in range(tile)] for p in range(H)])
    flat = np.sort(off.ravel())
    assert flat[0] == 0 and (np.diff(flat) == 96).all() and flat[-1] + 96 == H * tile * 96
    assert H * tile * 96 <= H * tile * 128
    for grp in range(H // 8):
        for t in range(tile):
            run = off[8 * grp: 8 * grp + 8, t]
            assert run[0] % 128 == 0 and (np.diff(run) == 96).all()
            assert run[0] == (grp * tile + t) * 768
