// cutbench -- what planning the cuts of a long recording costs on the device ("Measured"): the three launches of
// nh_cut_plan (k_cut.hip: frame energies, window energies, the cut search) on a device-resident recording, timed with HIP
// events on one stream, and the device-to-host copy of the recording that planning on the host would start with.
//   cutbench [seconds = 600] [reps = 20] [max_frames = 3000] [min_frames = 2000] [half_window = 15]
// The signal: noise bursts of 0.2 - 1.2 s separated by 0.5 s pauses (the content changes where the cuts fall, not the work).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../norma_amd/csrc/nh_kernels.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static double median(std::vector<float> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

int main(int argc, char **argv) {
    const long long seconds = argc > 1 ? atoll(argv[1]) : 600;
    const int reps = argc > 2 ? atoi(argv[2]) : 20;
    const int max_f = argc > 3 ? atoi(argv[3]) : 3000, min_f = argc > 4 ? atoi(argv[4]) : 2000, W = argc > 5 ? atoi(argv[5]) : 15;
    if (seconds < 1 || seconds > 100000 || reps < 1 || max_f < 1 || max_f > 3000 || min_f < 1 || min_f > max_f || W < 0 || W > 100) {
        fprintf(stderr, "usage: cutbench [seconds] [reps] [max_frames <= 3000] [min_frames <= max_frames] [half_window <= 100]\n");
        return 2;
    }
    const long long N = seconds * 16000, F = (N + NH_CUT_FRAME - 1) / NH_CUT_FRAME, cap = F / min_f + 1;
    std::vector<float> x((size_t)N);
    unsigned long long s = 88172645463325252ull;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (double)(s >> 11) * (1.0 / 9007199254740992.0); };
    for (long long at = 0; at < N;) {
        const long long b = 3200 + (long long)(rnd() * 16000);
        for (long long i = at; i < std::min(N, at + b); i++) x[(size_t)i] = (float)(0.6 * rnd() - 0.3);
        at += b;
        for (long long i = at; i < std::min(N, at + 8000); i++) x[(size_t)i] = (float)(2e-3 * rnd() - 1e-3);
        at += 8000;
    }
    float *pcm = nullptr, *e = nullptr, *E = nullptr;
    long long *starts = nullptr;
    int32_t *lens = nullptr, *count = nullptr;
    hipStream_t st;
    hipEvent_t ev[4];
    CK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    for (auto &v : ev) CK(hipEventCreate(&v));
    CK(hipMalloc(reinterpret_cast<void **>(&pcm), sizeof(float) * (size_t)N));
    CK(hipMalloc(reinterpret_cast<void **>(&e), sizeof(float) * (size_t)F));
    CK(hipMalloc(reinterpret_cast<void **>(&E), sizeof(float) * (size_t)F));
    CK(hipMalloc(reinterpret_cast<void **>(&starts), sizeof(long long) * (size_t)cap));
    CK(hipMalloc(reinterpret_cast<void **>(&lens), sizeof(int32_t) * (size_t)cap));
    CK(hipMalloc(reinterpret_cast<void **>(&count), sizeof(int32_t)));
    CK(hipMemcpy(pcm, x.data(), sizeof(float) * (size_t)N, hipMemcpyHostToDevice));
    CutSearch cs{};
    cs.E = E; cs.F = F; cs.min_frames = min_f; cs.max_frames = max_f; cs.n_samples = N;
    cs.starts = starts; cs.lens = lens; cs.count = count; cs.cap = cap;
    std::vector<float> all, k_e, k_w, k_s;
    for (int r = 0; r < reps + 2; r++) {   // two warm-ups
        CK(hipEventRecord(ev[0], st));
        launch_cut_energy(pcm, N, e, F, st);
        CK(hipEventRecord(ev[1], st));
        launch_cut_window(e, E, F, W, st);
        CK(hipEventRecord(ev[2], st));
        launch_cut_search(cs, st);
        CK(hipEventRecord(ev[3], st));
        CK(hipStreamSynchronize(st));
        CK(hipGetLastError());
        if (r < 2) continue;
        float a = 0, b = 0, c = 0, d = 0;
        CK(hipEventElapsedTime(&a, ev[0], ev[3]));
        CK(hipEventElapsedTime(&b, ev[0], ev[1]));
        CK(hipEventElapsedTime(&c, ev[1], ev[2]));
        CK(hipEventElapsedTime(&d, ev[2], ev[3]));
        all.push_back(a); k_e.push_back(b); k_w.push_back(c); k_s.push_back(d);
    }
    int32_t n = 0;
    CK(hipMemcpy(&n, count, sizeof(n), hipMemcpyDeviceToHost));
    std::vector<float> copy;
    for (int r = 0; r < std::min(reps, 5) + 1; r++) {   // the alternative's first step: the recording back to pageable host memory
        const auto t0 = std::chrono::steady_clock::now();
        CK(hipMemcpy(x.data(), pcm, sizeof(float) * (size_t)N, hipMemcpyDeviceToHost));
        if (r) copy.push_back(std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    printf("{\"seconds\": %lld, \"samples\": %lld, \"frames\": %lld, \"params\": [%d, %d, %d], \"chunks\": %d, \"reps\": %d, "
           "\"launches_us_median\": %.1f, \"launches_us_min\": %.1f, \"energy_us\": %.1f, \"window_us\": %.1f, \"search_us\": %.1f, "
           "\"energy_read_gb_per_s\": %.0f, \"copy_to_host_ms_median\": %.2f}\n",
           seconds, N, F, max_f, min_f, W, n, reps, 1e3 * median(all), 1e3 * *std::min_element(all.begin(), all.end()), 1e3 * median(k_e),
           1e3 * median(k_w), 1e3 * median(k_s), 4.0 * N / (median(k_e) * 1e-3) * 1e-9, median(copy));
    return 0;
}
