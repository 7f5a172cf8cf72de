// WKV6 sequence-kernel probe (tools/, not part of the library): times launch_wkv6 (head size 64,
// T = 1024, H = 32, per-token decay).
// Build: hipcc -std=c++17 -O3 --offload-arch=gfx950 -ffp-contract=off -DRWKV_BUILD
//        -Irwkv.cppy_amd/csrc -Iinclude -o tools/bin/wkv_probe tools/wkv_probe.hip
#include "wkv_serial.hip"

#include <stdlib.h>
#include <string.h>
#include <vector>

namespace rwkvmi { thread_local KLaunchTimer * g_klt = nullptr; }  // the library's is in engine.hip
using namespace rwkvmi;

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("err %s line %d\n", hipGetErrorString(e), __LINE__); exit(1); } } while (0)

int main() {
    const int T = 1024, H = 32, S = 64, C = H * S;
    std::vector<float> hk((size_t)T * C), hv(hk.size()), hr(hk.size()), hw(hk.size()), hu(C), hs((size_t)H * S * S);
    srand(1);
    auto rnd = [] { return (float)rand() / RAND_MAX - 0.5f; };
    for (size_t i = 0; i < hk.size(); i++) {
        hk[i] = rnd(); hv[i] = rnd(); hr[i] = rnd(); hw[i] = 0.9f + 0.1f * rnd();
    }
    for (auto & x : hu) x = rnd();
    for (auto & x : hs) x = rnd();
    float *k, *v, *r, *w, *u, *s0, *s1, *y;
    const size_t tb = hk.size() * 4;
    CK(hipMalloc(&k, tb)); CK(hipMalloc(&v, tb)); CK(hipMalloc(&r, tb)); CK(hipMalloc(&w, tb)); CK(hipMalloc(&y, tb));
    CK(hipMalloc(&u, C * 4)); CK(hipMalloc(&s0, hs.size() * 4)); CK(hipMalloc(&s1, hs.size() * 4));
    CK(hipMemcpy(k, hk.data(), tb, hipMemcpyHostToDevice)); CK(hipMemcpy(v, hv.data(), tb, hipMemcpyHostToDevice));
    CK(hipMemcpy(r, hr.data(), tb, hipMemcpyHostToDevice)); CK(hipMemcpy(w, hw.data(), tb, hipMemcpyHostToDevice));
    CK(hipMemcpy(u, hu.data(), C * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(s0, hs.data(), hs.size() * 4, hipMemcpyHostToDevice));
    hipStream_t st;
    CK(hipStreamCreate(&st));
    hipEvent_t a, b;
    CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    {
        for (int i = 0; i < 2; i++) launch_wkv6(st, T, H, S, k, v, r, u, w, 1, s0, s1, y);
        CK(hipEventRecord(a, st));
        const int reps = 10;
        for (int i = 0; i < reps; i++) launch_wkv6(st, T, H, S, k, v, r, u, w, 1, s0, s1, y);
        CK(hipEventRecord(b, st));
        CK(hipEventSynchronize(b));
        float ms;
        CK(hipEventElapsedTime(&ms, a, b));
        printf("wkv6 T=%d: %8.1f us\n", T, ms * 1e3 / reps);
    }
    return 0;
}
