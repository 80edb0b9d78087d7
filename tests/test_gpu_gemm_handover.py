"""GPU: the tile hand-over of gemm256_f16_kernel (k_gemm.hip) against the 128 x 128 kernel, byte for byte.

Both kernels accumulate a K-tile of 64 in the same order (the premise of tools/gemm_check.hip) and share the epilogue arithmetic,
so on the same inputs every output byte must agree; the 256 x 256 kernel's epilogues address their stores through a per-launch
row map, a buffer descriptor that ends with the launch's last row, and a bias row that travels through LDS with the next tile's
first fetches.  Output buffers are pre-filled with a sentinel and are longer than the launch writes: every byte outside the
written region -- rows >= M, the pad columns of the V^T image, the framing rows of the conv1 map -- must still hold it.
K = 128 throughout (two K-tiles: the shortest main loop the kernel has); the shapes are the smallest at which each path of the
hand-over can go wrong.  What the values should be is test_gpu_kernel_ref.py's business (fp64 references)."""
import zlib

import numpy as np
import pytest

import kref as K

pytestmark = pytest.mark.gpu

KD = 128
SENT16 = np.float16(7.25)
SENT32 = np.float32(-1234.5)


def rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _gemm(kernel128, A, lda, a_rpb, a_bstride, W, bias, M, epi, outs, seg_n, ldo, o_rpb=0, o_bstride=0, o_off=0, vt_seg=-1,
          head_major=0, seg0_scale=0.0, S=0, H=0):
    L = K.lib()
    N, Kd = W.shape
    o = list(outs) + [None] * (3 - len(outs))
    rc = L.kref_gemm(int(kernel128), K.ptr(A), A.nbytes, lda, a_rpb or M, a_bstride, K.ptr(W), K.ptr(bias), M, N, Kd, epi,
                     K.ptr(o[0]), K.ptr(o[1]), K.ptr(o[2]), outs[0].nbytes, seg_n, ldo, o_rpb or M, o_bstride, o_off, vt_seg,
                     head_major, seg0_scale, S, H, K.ptr(None))
    K.check_rc(rc, f"launch_gemm{'_128' if kernel128 else ''} M={M} N={N} K={Kd} epi={epi}")


def _operands(r, M, N, bias=True):
    A = K.f16(r.standard_normal((M, KD)))
    W = K.f16(r.standard_normal((N, KD)) / np.sqrt(KD))
    b = K.f32(r.standard_normal(N) * 0.5) if bias else None
    return A, W, b


def _both(fresh, launch):
    """the outputs of the 256 x 256 kernel and of the 128 x 128 kernel on buffers made by fresh()"""
    got = []
    for kernel128 in (0, 1):
        bufs = fresh()
        launch(kernel128, bufs)
        got.append(bufs)
    return got


def _same(a, b, what):
    ua, ub = a.view(np.uint8), b.view(np.uint8)
    bad = np.flatnonzero(ua.ravel() != ub.ravel())
    assert bad.size == 0, f"{what}: {bad.size} bytes differ between the 256 x 256 and the 128 x 128 kernel, first at byte {bad[0]}"


def _untouched(region, sentinel, what):
    assert np.all(region == sentinel), f"{what}: {int(np.count_nonzero(region != sentinel))} elements written"


def _written(region, sentinel, what):
    # a kernel that stored nothing would agree with itself: the written region must not be the sentinel
    assert np.count_nonzero(region == sentinel) <= region.size // 100, f"{what}: still holds the sentinel"


def test_qkv_three_segments_scaled_q_and_vt_with_clip_ends_inside_tiles_and_runs():
    """S = 100, M = 500: clip ends at rows 100 .. 400 fall inside the 256-row tiles and (100 % 8 = 4) inside 8-row V^T runs;
    the second tile is ragged (244 rows)"""
    M, N, seg_n, H, S = 500, 768, 256, 4, 100
    B = M // S
    A, W, bias = _operands(rng("ho-qkv"), M, N)
    rows = 512 + 8                                      # beyond the ragged tile's 512 rows
    n16 = max(rows * seg_n, (B + 1) * H * 64 * K.NH_SP)  # one size for the three buffers; the V^T image gets a sixth clip

    def fresh():
        return [np.full(n16, SENT16, np.float16) for _ in range(3)]

    def launch(kernel128, bufs):
        _gemm(kernel128, A, KD, M, 0, W, bias, M, K.EPI_F16, bufs, seg_n, seg_n, vt_seg=2, seg0_scale=K.ENC_Q_SCALE, S=S, H=H)

    g256, g128 = _both(fresh, launch)
    for i, name in enumerate(("q (scaled)", "k", "V^T")):
        _same(g256[i], g128[i], name)
    for i, name in enumerate(("q", "k")):
        _untouched(g256[i][M * seg_n:], SENT16, f"{name}: rows >= M")
        _written(g256[i][:M * seg_n], SENT16, name)
    vt = g256[2][:(B + 1) * H * 64 * K.NH_SP].reshape(B + 1, H, 64, K.NH_SP)
    _untouched(vt[:B, :, :, S:], SENT16, "V^T pad columns")
    _untouched(vt[B], SENT16, "V^T image of the clip after the last")
    _untouched(g256[2][vt.size:], SENT16, "behind the V^T image")
    _written(vt[:B, :, :, :S], SENT16, "V^T")
    # the scale reached q and only q
    assert not np.array_equal(g256[0][:M * seg_n], g256[1][:M * seg_n])


@pytest.mark.parametrize("M", [500, 257])
def test_head_major_two_outputs(M):
    """cross K/V, [b][h][S][64] with S = 100: several clip ends per tile; M = 257 leaves a one-row ragged tile, and the rows
    behind row M - 1 of the last clip lie INSIDE the allocation (the next head's rows follow): only the descriptor's end, the
    launch's last row, keeps them"""
    N, seg_n, H, S = 512, 256, 4, 100
    B = -(-M // S)
    A, W, bias = _operands(rng("ho-hm", M), M, N)
    n16 = (B + 1) * H * S * 64

    def fresh():
        return [np.full(n16, SENT16, np.float16) for _ in range(2)]

    def launch(kernel128, bufs):
        _gemm(kernel128, A, KD, M, 0, W, bias, M, K.EPI_F16, bufs, seg_n, seg_n, head_major=1, S=S, H=H)

    g256, g128 = _both(fresh, launch)
    for i, name in enumerate(("cross k", "cross v")):
        _same(g256[i], g128[i], f"{name} M={M}")
        img = g256[i].reshape(B + 1, H, S, 64)
        valid = (np.arange(B + 1)[:, None] * S + np.arange(S)[None, :]) < M          # [b][s]: row b S + s exists
        mask = np.broadcast_to(valid[:, None, :, None], img.shape)
        _untouched(img[~mask], SENT16, f"{name} M={M}: rows >= M")
        _written(img[mask], SENT16, f"{name} M={M}")


@pytest.mark.parametrize("M", [256, 257, 511])
def test_gelu_prefill_form(M):
    """EPI_GELU_F16 with S = M = a_rpb = o_rpb (every magic 0): one full tile, a one-row ragged tile, a tile one row short"""
    N = 256
    A, W, bias = _operands(rng("ho-gelu", M), M, N)
    rows = 512 + 8

    def fresh():
        return [np.full(rows * N, SENT16, np.float16)]

    def launch(kernel128, bufs):
        _gemm(kernel128, A, KD, M, 0, W, bias, M, K.EPI_GELU_F16, bufs, N, N, o_rpb=M, S=M, H=4)

    g256, g128 = _both(fresh, launch)
    _same(g256[0], g128[0], f"gelu M={M}")
    _untouched(g256[0][M * N:], SENT16, f"gelu M={M}: rows >= M")
    _written(g256[0][:M * N], SENT16, f"gelu M={M}")


def test_gelu_without_bias():
    """no bias: the epilogue reads the zeroed bias rows"""
    M, N = 257, 256
    A, W, _ = _operands(rng("ho-nobias"), M, N, bias=False)

    def fresh():
        return [np.full(520 * N, SENT16, np.float16)]

    def launch(kernel128, bufs):
        _gemm(kernel128, A, KD, M, 0, W, None, M, K.EPI_GELU_F16, bufs, N, N, o_rpb=M, S=M, H=4)

    g256, g128 = _both(fresh, launch)
    _same(g256[0], g128[0], "gelu without bias")
    _untouched(g256[0][M * N:], SENT16, "gelu without bias: rows >= M")


def test_conv1_row_map():
    """conv1's maps at F = 200, B = 3: A rows inside [F + 2]-row frames, output rows offset by one inside [F + 2]-row frames;
    F < 256, so every tile holds a frame end, the last one two with the end of M"""
    F, B, N = 200, 3, 256
    M = B * F
    r = rng("ho-conv1")
    mel = K.f16(r.standard_normal((B, F + 2, KD)))
    W = K.f16(r.standard_normal((N, KD)) / np.sqrt(KD))
    bias = K.f32(r.standard_normal(N) * 0.5)

    def fresh():
        return [np.full((B + 1) * (F + 2) * N, SENT16, np.float16)]

    def launch(kernel128, bufs):
        _gemm(kernel128, mel, KD, F, (F + 2) * KD, W, bias, M, K.EPI_GELU_F16, bufs, N, N, o_rpb=F, o_bstride=F + 2, o_off=1, S=F // 2, H=4)

    g256, g128 = _both(fresh, launch)
    _same(g256[0], g128[0], "conv1")
    h1 = g256[0].reshape(B + 1, F + 2, N)
    _untouched(h1[:B, 0], SENT16, "conv1: first framing row")
    _untouched(h1[:B, F + 1], SENT16, "conv1: last framing row")
    _untouched(h1[B], SENT16, "conv1: frame after the last clip")
    _written(h1[:B, 1:F + 1], SENT16, "conv1")


def test_residual_one_row_ragged_tile():
    M, N = 257, 256
    r = rng("ho-resid")
    A, W, bias = _operands(r, M, N)
    x0 = np.full((520, N), SENT32, np.float32)
    x0[:M] = K.f32(r.standard_normal((M, N)))

    def fresh():
        return [x0.copy().ravel()]

    def launch(kernel128, bufs):
        _gemm(kernel128, A, KD, M, 0, W, bias, M, K.EPI_RESID_F32, bufs, N, N)

    g256, g128 = _both(fresh, launch)
    _same(g256[0], g128[0], "residual")
    _untouched(g256[0][M * N:], SENT32, "residual: rows >= M")
    assert np.count_nonzero(g256[0][:M * N] == x0[:M].ravel()) <= M * N // 100, "residual: nothing added"


def test_more_tiles_than_workgroups():
    """280 tiles on at most 256 workgroups: some workgroups hand over from one tile to the next, with the bias row changing"""
    M, N = 2305, 7168
    A, W, bias = _operands(rng("ho-many"), M, N)
    rows = 2560 + 8

    def fresh():
        return [np.full(rows * N, SENT16, np.float16)]

    def launch(kernel128, bufs):
        _gemm(kernel128, A, KD, M, 0, W, bias, M, K.EPI_F16, bufs, N, N, o_rpb=M, S=M, H=4)

    g256, g128 = _both(fresh, launch)
    _same(g256[0], g128[0], "fp16, 280 tiles")
    _untouched(g256[0][M * N:], SENT16, "fp16, 280 tiles: rows >= M")
    _written(g256[0][:M * N], SENT16, "fp16, 280 tiles")
