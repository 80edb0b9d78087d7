// vadbench -- what the speech map of a long recording costs on the device ("Measured"): the launches of nh_vad_plan
// (k_cut.hip's energies, then k_vad.hip: the select, the shaping scans, the region list, the piece walk) on a device-resident
// recording, timed per stage with HIP events on one stream; then the gather of the planned chunks into PCM rows, one launch
// (table copy included) against one device-to-device hipMemcpyAsync per piece.
//   vadbench [seconds = 600] [reps = 20] [max_frames = 3000] [min_frames = 2000] [half_window = 15] [min_speech = 10] [pad = 20] [min_gap = 100]
// The signal: noise bursts of 0.2 - 1.2 s at 0.3 with pauses of 0.5 s or, one time in four, 3 s at 1e-3.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../norma_amd/csrc/nh_kernels.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static double median(std::vector<float> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }
template <class T> static hipError_t dmalloc(T **p, size_t n) { return hipMalloc(reinterpret_cast<void **>(p), sizeof(T) * std::max<size_t>(n, 1)); }

int main(int argc, char **argv) {
    const long long seconds = argc > 1 ? atoll(argv[1]) : 600;
    const int reps = argc > 2 ? atoi(argv[2]) : 20;
    const int max_f = argc > 3 ? atoi(argv[3]) : 3000, min_f = argc > 4 ? atoi(argv[4]) : 2000, W = argc > 5 ? atoi(argv[5]) : 15;
    const int min_speech = argc > 6 ? atoi(argv[6]) : 10, pad = argc > 7 ? atoi(argv[7]) : 20, min_gap = argc > 8 ? atoi(argv[8]) : 100;
    if (seconds < 1 || seconds > 100000 || reps < 1 || max_f < 1 || max_f > 3000 || min_f < 1 || min_f > max_f || W < 0 || W > 100 ||
        min_speech < 1 || pad < 0 || min_gap < 1) {
        fprintf(stderr, "usage: vadbench [seconds] [reps] [max_frames <= 3000] [min_frames <= max_frames] [half_window <= 100] [min_speech] [pad] [min_gap]\n");
        return 2;
    }
    const long long N = seconds * 16000, F = (N + NH_CUT_FRAME - 1) / NH_CUT_FRAME;
    const long long n_tiles = (F + NH_VAD_TILE - 1) / NH_VAD_TILE, Fp = n_tiles * NH_VAD_TILE, max_regions = F / 2 + 1;
    const long long cap = max_regions + F / min_f + 1;
    std::vector<float> x((size_t)N);
    unsigned long long s = 88172645463325252ull;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (double)(s >> 11) * (1.0 / 9007199254740992.0); };
    long long quiet = 0;
    for (long long at = 0; at < N;) {
        const long long b = 3200 + (long long)(rnd() * 16000), p = rnd() < 0.25 ? 48000 : 8000;
        for (long long i = at; i < std::min(N, at + b); i++) x[(size_t)i] = (float)(0.6 * rnd() - 0.3);
        at += b;
        for (long long i = at; i < std::min(N, at + p); i++, quiet++) x[(size_t)i] = (float)(2e-3 * rnd() - 1e-3);
        at += p;
    }
    float *pcm = nullptr, *e = nullptr, *E = nullptr, *levels = nullptr, *rows = nullptr;
    VadSelect *sel = nullptr;
    uint8_t *flags = nullptr;
    int *tiles = nullptr, *n_regions = nullptr;
    long long *regions = nullptr, *starts = nullptr, *tab = nullptr;
    int32_t *lens = nullptr, *first = nullptr, *counts = nullptr;
    hipStream_t st;
    hipEvent_t ev[6];
    CK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    for (auto &v : ev) CK(hipEventCreate(&v));
    CK(dmalloc(&pcm, (size_t)N)); CK(dmalloc(&e, (size_t)F)); CK(dmalloc(&E, (size_t)F)); CK(dmalloc(&levels, 4)); CK(dmalloc(&sel, 1));
    CK(dmalloc(&flags, 3 * (size_t)Fp)); CK(dmalloc(&tiles, 4 * (size_t)n_tiles)); CK(dmalloc(&n_regions, 1));
    CK(dmalloc(&regions, 2 * (size_t)max_regions)); CK(dmalloc(&starts, (size_t)cap)); CK(dmalloc(&lens, (size_t)cap));
    CK(dmalloc(&first, (size_t)cap + 1)); CK(dmalloc(&counts, 2));
    CK(hipMemcpy(pcm, x.data(), sizeof(float) * (size_t)N, hipMemcpyHostToDevice));
    const VadLevels lv{100, 900, 4.0f, 0.01f, 0.0f};
    uint8_t *const f0 = flags, *const f1 = flags + Fp, *const v3 = flags + 2 * Fp;
    VadShape sh{};
    sh.E = E; sh.levels = levels; sh.F = F; sh.tile_l = tiles; sh.tile_r = tiles + n_tiles; sh.carry_l = tiles + 2 * n_tiles;
    sh.carry_r = tiles + 3 * n_tiles; sh.min_speech = min_speech; sh.pad = pad; sh.min_gap = min_gap; sh.regions = regions; sh.carry_n = sh.carry_l;
    const uint8_t *const ins[6] = {nullptr, f0, f1, f0, v3, v3};
    uint8_t *const outs[6] = {f0, f1, f0, v3, nullptr, nullptr};
    VadPieces pc{};
    pc.E = E; pc.regions = regions; pc.n_regions = n_regions; pc.min_frames = min_f; pc.max_frames = max_f; pc.n_samples = N;
    pc.starts = starts; pc.lens = lens; pc.cap_pieces = cap; pc.chunk_first = first; pc.cap_chunks = cap; pc.counts = counts;
    auto shape = [&](int step) {
        sh.in = ins[step]; sh.out = outs[step];
        launch_vad_shape(step, sh, st);
        if (step <= 2) launch_vad_carry(sh.tile_l, sh.tile_r, tiles + 2 * n_tiles, tiles + 3 * n_tiles, (int)n_tiles, F, 0, nullptr, st);
        if (step == 4) launch_vad_carry(sh.tile_l, sh.tile_r, tiles + 2 * n_tiles, tiles + 3 * n_tiles, (int)n_tiles, F, 1, n_regions, st);
    };
    std::vector<float> t_all, t_stage[5];
    for (int r = 0; r < reps + 2; r++) {   // two warm-ups
        CK(hipEventRecord(ev[0], st));
        CK(hipMemsetAsync(sel, 0, sizeof(VadSelect), st));
        launch_cut_energy(pcm, N, e, F, st);
        launch_cut_window(e, E, F, W, st);
        CK(hipEventRecord(ev[1], st));
        for (int shift = 24; shift >= 0; shift -= 8) { launch_vad_hist(E, F, shift, sel, st); launch_vad_pick(sel, shift, lv, levels, st); }
        CK(hipEventRecord(ev[2], st));
        for (int step = 0; step <= 3; step++) shape(step);
        CK(hipEventRecord(ev[3], st));
        shape(4); shape(5);
        CK(hipEventRecord(ev[4], st));
        launch_vad_pieces(pc, st);
        CK(hipEventRecord(ev[5], st));
        CK(hipStreamSynchronize(st));
        CK(hipGetLastError());
        if (r < 2) continue;
        float a = 0;
        CK(hipEventElapsedTime(&a, ev[0], ev[5]));
        t_all.push_back(a);
        for (int k = 0; k < 5; k++) { CK(hipEventElapsedTime(&a, ev[k], ev[k + 1])); t_stage[k].push_back(a); }
    }
    int32_t n[2] = {0, 0}, nr = 0;
    float h_levels[3];
    CK(hipMemcpy(n, counts, sizeof(n), hipMemcpyDeviceToHost));
    CK(hipMemcpy(&nr, n_regions, sizeof(nr), hipMemcpyDeviceToHost));
    CK(hipMemcpy(h_levels, levels, sizeof(h_levels), hipMemcpyDeviceToHost));
    std::vector<long long> h_starts((size_t)n[0]);
    std::vector<int32_t> h_lens((size_t)n[0]), h_first((size_t)n[1] + 1);
    CK(hipMemcpy(h_starts.data(), starts, sizeof(long long) * h_starts.size(), hipMemcpyDeviceToHost));
    CK(hipMemcpy(h_lens.data(), lens, sizeof(int32_t) * h_lens.size(), hipMemcpyDeviceToHost));
    CK(hipMemcpy(h_first.data(), first, sizeof(int32_t) * h_first.size(), hipMemcpyDeviceToHost));
    long long kept = 0;
    for (int32_t v : h_lens) kept += v;
    // the gather: the first `batch` chunks into rows of 480 000 floats, both ways
    const int batch = std::min(n[1], 32), P = batch > 0 ? h_first[(size_t)batch] : 0;
    std::vector<float> t_gather, t_copies;
    if (batch > 0) {
        std::vector<long long> h_tab((size_t)(batch + 1) + 2 * (size_t)P + (size_t)batch);
        long long *t_first = h_tab.data(), *t_src = t_first + batch + 1, *t_off = t_src + P, *t_tot = t_off + P, max_total = 0;
        for (int b = 0; b < batch; b++) {
            t_first[b] = h_first[(size_t)b];
            long long at = 0;
            for (int j = h_first[(size_t)b]; j < h_first[(size_t)b + 1]; j++) { t_src[j] = h_starts[(size_t)j]; t_off[j] = at; at += h_lens[(size_t)j]; }
            t_tot[b] = at;
            max_total = std::max(max_total, at);
        }
        t_first[batch] = P;
        CK(dmalloc(&rows, (size_t)batch * 480000)); CK(dmalloc(&tab, h_tab.size()));
        VadGather g{};
        g.src = pcm; g.dst = rows; g.dst_stride = 480000; g.tab = tab; g.n_pieces = P; g.vec4 = 1;   // a plan's pieces: multiples of 160 samples
        for (int r = 0; r < reps + 2; r++) {
            CK(hipEventRecord(ev[0], st));
            CK(hipMemcpyAsync(tab, h_tab.data(), sizeof(long long) * h_tab.size(), hipMemcpyHostToDevice, st));
            launch_vad_gather(g, batch, max_total, st);
            CK(hipEventRecord(ev[1], st));
            for (int b = 0; b < batch; b++)
                for (int j = h_first[(size_t)b]; j < h_first[(size_t)b + 1]; j++)
                    CK(hipMemcpyAsync(rows + (size_t)b * 480000 + t_off[j], pcm + t_src[j], sizeof(float) * (size_t)h_lens[(size_t)j], hipMemcpyDeviceToDevice, st));
            CK(hipEventRecord(ev[2], st));
            CK(hipStreamSynchronize(st));
            CK(hipGetLastError());
            if (r < 2) continue;
            float a = 0, b2 = 0;
            CK(hipEventElapsedTime(&a, ev[0], ev[1]));
            CK(hipEventElapsedTime(&b2, ev[1], ev[2]));
            t_gather.push_back(a); t_copies.push_back(b2);
        }
    }
    long long bytes = 0;
    for (int j = 0; j < P; j++) bytes += 4ll * h_lens[(size_t)j];
    printf("{\"seconds\": %lld, \"samples\": %lld, \"frames\": %lld, \"quiet_samples\": %lld, \"params\": [%d, %d, %d, %d, %d, %d], \"levels\": [%g, %g, %g], "
           "\"regions\": %d, \"pieces\": %d, \"chunks\": %d, \"kept_samples\": %lld, \"reps\": %d, \"launches_us_median\": %.1f, \"launches_us_min\": %.1f, "
           "\"energies_us\": %.1f, \"select_us\": %.1f, \"scans_us\": %.1f, \"regions_us\": %.1f, \"pieces_us\": %.1f, "
           "\"gather_chunks\": %d, \"gather_pieces\": %d, \"gather_mb\": %.1f, \"gather_one_launch_us\": %.1f, \"gather_copy_per_piece_us\": %.1f}\n",
           seconds, N, F, quiet, max_f, min_f, W, min_speech, pad, min_gap, h_levels[0], h_levels[1], h_levels[2], nr, n[0], n[1], kept, reps,
           1e3 * median(t_all), 1e3 * *std::min_element(t_all.begin(), t_all.end()), 1e3 * median(t_stage[0]), 1e3 * median(t_stage[1]),
           1e3 * median(t_stage[2]), 1e3 * median(t_stage[3]), 1e3 * median(t_stage[4]), batch, P, bytes * 1e-6,
           batch ? 1e3 * median(t_gather) : 0.0, batch ? 1e3 * median(t_copies) : 0.0);
    return 0;
}
