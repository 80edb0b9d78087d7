// mel_host.h -- the host half of the log-mel front end (k_mel.hip): the tables logmel_kernel reads and the per-filter group
// range its filter sum walks.  Pure host code, no HIP: nh_model.hip uploads what these return, and tools/kref.hip hands the same
// values to the kernel-level tests, so that a test's tables are the product's and not a copy.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#define MEL_N_HANN 400
#define MEL_N_DFT 625   // [25][25]
#define MEL_N_TW 375    // radix-2 twiddles for n = 50, 100, 200, 400 at offsets 0, 25, 75, 175 (k < n / 2)

// host tables with libm, the same f32 expressions candle evaluates (see k_mel.hip); tw_sin holds -sin(theta)
static inline void mel_host_tables(float *hann, float *dc, float *dsn, float *twc, float *tws) {
    const float two_pi = (float)M_PI + (float)M_PI;
    for (int i = 0; i < 400; i++) hann[i] = 0.5f * (1.0f - cosf((two_pi * (float)i) / 400.0f));
    for (int k = 0; k < 25; k++)
        for (int j = 0; j < 25; j++) {
            float angle = two_pi * (float)k * (float)j / 25.0f;
            dc[k * 25 + j] = cosf(angle); dsn[k * 25 + j] = sinf(angle);
        }
    int off = 0;
    for (int h = 25; h <= 200; h *= 2) {
        float n_t = (float)(2 * h);
        for (int k = 0; k < h; k++) {
            float theta = two_pi * (float)k / n_t;
            twc[off + k] = cosf(theta); tws[off + k] = -sinf(theta);
        }
        off += h;
    }
}

// grp [n_mel][2]: first / last + 1 group of four bins (of the 50 below bin 200) in which filter m [201] has a non-zero tap
static inline void mel_host_groups(const float *filters, int n_mel, int32_t *grp) {
    for (int m = 0; m < n_mel; m++) {
        int g0 = 50, g1 = 0;
        for (int g = 0; g < 50; g++) {
            bool nz = false;
            for (int k = 4 * g; k < 4 * g + 4; k++) nz = nz || filters[(size_t)m * 201 + k] != 0.f;
            if (nz) { if (g < g0) g0 = g; g1 = g + 1; }
        }
        if (g0 > g1) g0 = g1 = 0;
        grp[2 * m] = g0; grp[2 * m + 1] = g1;
    }
}
