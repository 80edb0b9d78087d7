// kref_score.hip -- test-only C entry points onto launch_score_rows (k_score.hip) on raw device buffers (tests/score_ref.py,
// tests/test_gpu_score_kernel.py).  Linked against the library's own object: the kernels under test are the product's.
// Host buffers in, device copies made, one launch on a stream of its own, the outputs copied back.  Returns the hipError_t,
// or -1 when the launcher refuses the shape.
#include <vector>

#include "../norma_amd/csrc/nh_kernels.h"

namespace {
struct Dev {
    std::vector<void *> bufs;
    hipError_t err = hipSuccess;
    void *make(size_t bytes, const void *host, int fill) {
        if (err != hipSuccess) return nullptr;
        void *d = nullptr;
        if ((err = hipMalloc(&d, bytes ? bytes : 16)) != hipSuccess) return nullptr;
        bufs.push_back(d);
        if (host) err = hipMemcpy(d, host, bytes, hipMemcpyHostToDevice);
        else err = hipMemset(d, fill, bytes);
        return d;
    }
    ~Dev() {
        for (void *d : bufs) (void)hipFree(d);
    }
};

// xn holds xn_bytes >= M * d * 2 bytes and E e_bytes >= V * d * 2: what lies past the M rows / V rows is the test's guard
// region, uploaded as it is, right behind the operands.  out f32 [M]: rows with targets[m] < 0 keep what they held.
int score_rows(const void *xn, size_t xn_bytes, int M, int d, const void *E, size_t e_bytes, int V, const int32_t *targets, float *out,
               int panel_rows) {
    if (M < 1 || V < 1 || d < 1 || xn_bytes < (size_t)M * d * 2 || e_bytes < (size_t)V * d * 2) return -1;
    Dev dv;
    const int panel = panel_rows > 0 ? panel_rows : score_panel_rows(V);
    const size_t rows = (size_t)(M < panel ? M : panel), ntn = ((size_t)V + 127) / 128;
    const half_t *dxn = static_cast<const half_t *>(dv.make(xn_bytes, xn, 0)), *dE = static_cast<const half_t *>(dv.make(e_bytes, E, 0));
    const int32_t *dt = static_cast<const int32_t *>(dv.make((size_t)M * 4, targets, 0));
    float *dout = static_cast<float *>(dv.make((size_t)M * 4, out, 0));
    // the scratch starts as NaN: a partial or a target logit read before it was written shows
    float *dpart = static_cast<float *>(dv.make(rows * ntn * 8, nullptr, 0xff)), *dtl = static_cast<float *>(dv.make((size_t)M * 4, nullptr, 0xff));
    if (dv.err != hipSuccess) return (int)dv.err;
    hipStream_t st = nullptr;
    if (hipError_t e = hipStreamCreate(&st)) return (int)e;   // a blocking stream: ordered after the copies above
    const bool launched = launch_score_rows(dxn, M, d, dE, V, dt, dpart, dtl, M, 0, 0, dout, panel_rows, st);
    hipError_t e = hipGetLastError(), e2 = hipStreamSynchronize(st);
    (void)hipStreamDestroy(st);
    if (e != hipSuccess) return (int)e;
    if (e2 != hipSuccess) return (int)e2;
    if (!launched) return -1;
    return (int)hipMemcpy(out, dout, (size_t)M * 4, hipMemcpyDeviceToHost);
}
}  // namespace

extern "C" {
// the two kernels on M rows: out[m] = log softmax(xn[m] . E^T)[targets[m]]
int kref_score_rows(const void *xn, size_t xn_bytes, int M, int d, const void *E, size_t e_bytes, int V, const int32_t *targets, float *out) {
    return score_rows(xn, xn_bytes, M, d, E, e_bytes, V, targets, out, 0);
}
// the same with the rows cut into panels of panel_rows (a multiple of 128): the loop a call with more rows than
// score_panel_rows(V) takes, at a size a test can afford
int kref_score_rows_panels(const void *xn, size_t xn_bytes, int M, int d, const void *E, size_t e_bytes, int V, const int32_t *targets,
                           float *out, int panel_rows) {
    return score_rows(xn, xn_bytes, M, d, E, e_bytes, V, targets, out, panel_rows);
}
int kref_score_panel_rows(int V) { return score_panel_rows(V); }
}
