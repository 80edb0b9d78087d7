"""Alignment from the decode (nh_align_capture / nh_align_decoded): the ctypes signatures of the test-only entry points of
tools/kref.hip for the capture kernel (launch_align_qsave) and for the row-mapped stage launchers, and a numpy statement
of what the capture kernel may write."""
import ctypes as C

import numpy as np

import kref as K
from align_ref import i32


def lib():
    L = K.lib()
    if L.kref_align_qsave_rows.argtypes is None:
        vp, i = C.c_void_p, C.c_int
        for n in ("kref_align_qsave_rows", "kref_align_weights_rows", "kref_align_reduce_rows", "kref_align_dtw_rows"):
            getattr(L, n).restype = C.c_int
        L.kref_align_qsave_rows.argtypes = [vp, vp, vp, i, i, i, i, i, vp, vp, i]
        L.kref_align_weights_rows.argtypes = [vp, vp, vp, i, i, i, i, vp, i, vp, vp, i, vp]
        L.kref_align_reduce_rows.argtypes = [vp, i, i, i, i, vp, vp, vp, i, vp]
        L.kref_align_dtw_rows.argtypes = [vp, i, i, i, vp, vp, vp, i, vp, vp, i]
    return L


def nan_pattern(shape):
    """fp16 NaNs with a payload that differs from cell to cell: a cell the kernel must leave alone keeps ITS pattern"""
    n = int(np.prod(shape))
    return (np.uint16(0x7E00) | (np.arange(n, dtype=np.uint32) % 0x1FF + 1).astype(np.uint16)).reshape(shape)


def gpu_qsave_rows(dq, qlive_bits, heads, ldb, npos, pos=0, pos_ptr=None, done=None):
    """dq fp16 [B][d]; qlive_bits u16 [len(heads)][npos][ldb][64] (the buffer as bits, copied in and back)"""
    B, d = dq.shape
    dq, heads = K.f16(dq), i32(heads)
    out = np.ascontiguousarray(qlive_bits, dtype=np.uint16).copy()
    pp = None if pos_ptr is None else i32(pos_ptr)
    dn = None if done is None else i32(done)
    rc = lib().kref_align_qsave_rows(K.ptr(dq), K.ptr(out), K.ptr(heads), len(heads), B, ldb, d, int(pos), K.ptr(pp), K.ptr(dn), npos)
    K.check_rc(rc, "kref_align_qsave_rows")
    return out


def qsave_rows_expected(dq, qlive_bits, heads, npos, pos=0, pos_ptr=None, done=None):
    """the contract: row b is written at its position iff done[b] == 0 and 0 <= position < npos; nothing else changes"""
    want = np.array(qlive_bits, dtype=np.uint16, copy=True)
    bits = K.f16(dq).view(np.uint16)
    for b in range(dq.shape[0]):
        p = int(pos if pos_ptr is None else pos_ptr[b])
        if (done is not None and done[b] != 0) or p < 0 or p >= npos:
            continue
        for a, h in enumerate(heads):
            want[a, p, b] = bits[b, 64 * h:64 * h + 64]
    return want


def gpu_weights_rows(q, k, heads, row_map, n_rows, n_keys, fill=np.nan):
    """q fp16 [A][max_rows][B][64], k fp16 [B][H][S][64], row_map [n] or None -> W f32 [n][A][max_rows][S]"""
    A, max_rows, B, _ = q.shape
    H, S = k.shape[1], k.shape[2]
    n = len(n_rows)
    W = np.full((n, A, max_rows, S), fill, dtype=np.float32)
    q, k, heads, n_rows, n_keys = K.f16(q), K.f16(k), i32(heads), i32(n_rows), i32(n_keys)
    rm = None if row_map is None else i32(row_map)
    rc = lib().kref_align_weights_rows(K.ptr(q), K.ptr(k), K.ptr(heads), A, H, S, B, K.ptr(rm), n, K.ptr(n_rows), K.ptr(n_keys), max_rows, K.ptr(W))
    K.check_rc(rc, "kref_align_weights_rows")
    return W


def gpu_reduce_rows(W, row_map, n_rows, n_keys, P, fill=np.nan):
    """W f32 [n][A][max_rows][S] -> M f32 [n][max_rows][S]"""
    n, A, max_rows, S = W.shape
    M = np.full((n, max_rows, S), fill, dtype=np.float32)
    W, n_rows, n_keys = K.f32(W), i32(n_rows), i32(n_keys)
    rm = None if row_map is None else i32(row_map)
    rc = lib().kref_align_reduce_rows(K.ptr(W), A, n, S, max_rows, K.ptr(rm), K.ptr(n_rows), K.ptr(n_keys), P, K.ptr(M))
    K.check_rc(rc, "kref_align_reduce_rows")
    return M


def gpu_dtw_rows(M, row_map, n_rows, n_keys, P):
    """M f32 [n][max_rows][S] -> first, last i32 [n][max_rows + 1]"""
    n, max_rows, S = M.shape
    ldo = max_rows + 1
    first, last = np.full((n, ldo), -7, np.int32), np.full((n, ldo), -7, np.int32)
    M, n_rows, n_keys = K.f32(M), i32(n_rows), i32(n_keys)
    rm = None if row_map is None else i32(row_map)
    rc = lib().kref_align_dtw_rows(K.ptr(M), n, S, max_rows, K.ptr(rm), K.ptr(n_rows), K.ptr(n_keys), P, K.ptr(first), K.ptr(last), ldo)
    K.check_rc(rc, "kref_align_dtw_rows")
    return first, last
