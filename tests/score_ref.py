"""Reference for the two scoring kernels (norma_amd/csrc/k_score.hip), driven through
tools/bin/libnh_kref_score.so (tools/kref_score.hip: C entry points onto launch_score_rows on raw device buffers).

The reference is the fp64 log-softmax at the target column from the exact fp16 operands the kernel was given.  The bound is
derived from the kernel's arithmetic, the way tests/kref.py and tests/beam_ref.py derive theirs; it is not measured.

    device = (float)((double)(l[t] - m) - log((double)se)),  l[v] = sum_k xn[k] E[v][k] in f32, m = max_v l,
    se = sum_v exp(l[v] - m) in f32 (per 128-column tile against the tile's maximum, the tiles merged by rescaling)

  * the logit term.  Every l[v] is an f32 accumulation of K = d products (MFMA chains, 32-deep steps in ascending order):
    |l[v] - exact| <= a[v] = kref.acc_bound(sum_k |xn_k E_vk|, K) = 2 K u sum_k |xn_k E_vk|.  The result is l[t] - logsumexp(l),
    and logsumexp moves by at most max_v of what its arguments move (its gradient is a probability vector), so the two
    together are within a[t] + max_v a[v].
  * the softmax term.  beam_ref.LOGQ_BOUND = 2e-5 covers an f32 softmax sum over at most 65536 fast-exp terms against the row
    maximum.  The tile form adds, per tile, one fast exp of (tile maximum - row maximum) and one product, and at most
    ceil(406 / 64) + 6 merges of two roundings each: 1.3e-6 + 6e-8 + 13 * 1.2e-7 < 3.1e-6 relative on se, inside the factor of
    two that LOGQ_BOUND already holds over its own 8e-6.  A tile further than 30 below the row maximum carries less than
    e^-30 of se whatever its scale factor's error.
  * the subtraction l[t] - m rounds once in f32: u |l[t] - m| <= u (|ref| + ln 65536), because 0 <= log se <= ln 65536; the
    final conversion to f32 rounds once more: u |ref|.  The double-precision tail adds nothing visible.
"""
import ctypes as C
import math
import os

import numpy as np

import beam_ref
import kref

LIB_PATH = os.path.join(kref.ROOT, "tools", "bin", "libnh_kref_score.so")
NAN16 = np.uint16(0x7e00)   # an fp16 quiet NaN
_lib = None


def lib():
    """The wrapper library; a GPU run without it FAILS (pytest.fail): a vacuous pass is not a pass."""
    global _lib
    if _lib is None:
        import pytest
        if not os.path.exists(LIB_PATH):
            pytest.fail(f"{LIB_PATH} is not built (python -c 'import __graft_entry__ as g; g.build()')")
        L = C.CDLL(LIB_PATH)
        vp, i, z = C.c_void_p, C.c_int, C.c_size_t
        L.kref_score_rows.argtypes = [vp, z, i, i, vp, z, i, vp, vp]
        L.kref_score_rows_panels.argtypes = [vp, z, i, i, vp, z, i, vp, vp, i]
        L.kref_score_panel_rows.argtypes = [i]
        for n in ("kref_score_rows", "kref_score_rows_panels", "kref_score_panel_rows"):
            getattr(L, n).restype = C.c_int
        _lib = L
    return _lib


def guarded(a16, guard_rows):
    """The fp16 rows of `a16` followed by `guard_rows` rows of NaN, as the uint16 image the device buffer gets."""
    a = np.ascontiguousarray(a16, dtype=np.float16)
    out = np.full((a.shape[0] + guard_rows, a.shape[1]), NAN16, dtype=np.uint16)
    out[:a.shape[0]] = a.view(np.uint16)
    return out


def score_rows(xn_img, M, d, E_img, V, targets, panel_rows=0, fill=np.nan):
    """kref_score_rows on the first M rows of xn_img and the first V of E_img (what follows them is uploaded as it is: the
    guard regions).  Returns f32 [M]; rows whose target is < 0 keep `fill`."""
    t = np.ascontiguousarray(targets, dtype=np.int32)
    assert len(t) == M
    out = np.full(M, fill, dtype=np.float32)
    L = lib()
    if panel_rows:
        rc = L.kref_score_rows_panels(kref.ptr(xn_img), xn_img.nbytes, M, d, kref.ptr(E_img), E_img.nbytes, V, kref.ptr(t), kref.ptr(out), panel_rows)
    else:
        rc = L.kref_score_rows(kref.ptr(xn_img), xn_img.nbytes, M, d, kref.ptr(E_img), E_img.nbytes, V, kref.ptr(t), kref.ptr(out))
    assert rc == 0, f"kref_score_rows: {rc}"
    return out


class Reference:
    """fp64 statistics of the rows of one (xn, E) pair, computed once and shared: logsumexp of every row and the largest
    accumulation bound of any column, in row blocks so that no [M][V] fp64 matrix is kept."""

    def __init__(self, xn16, E16):
        self.x = np.asarray(xn16, dtype=np.float64)
        self.E16 = np.ascontiguousarray(E16, dtype=np.float16)
        self.K = self.x.shape[1]
        Et = self.E16.astype(np.float64).T
        Eat = np.abs(Et)
        self.lse = np.empty(len(self.x))
        self.amax = np.empty(len(self.x))
        for r0 in range(0, len(self.x), 64):
            l = self.x[r0:r0 + 64] @ Et
            m = l.max(axis=1, keepdims=True)
            self.lse[r0:r0 + 64] = (m + np.log(np.exp(l - m).sum(axis=1, keepdims=True)))[:, 0]
            self.amax[r0:r0 + 64] = kref.acc_bound((np.abs(self.x[r0:r0 + 64]) @ Eat).max(axis=1), self.K)

    def at(self, m, t):
        """(reference, bound) of row m at target column t"""
        e = self.E16[t].astype(np.float64)
        ref = float(self.x[m] @ e) - float(self.lse[m])
        a_t = kref.acc_bound(float(np.abs(self.x[m]) @ np.abs(e)), self.K)
        return ref, a_t + float(self.amax[m]) + beam_ref.LOGQ_BOUND + kref.U32 * (2.0 * abs(ref) + math.log(65536.0))
