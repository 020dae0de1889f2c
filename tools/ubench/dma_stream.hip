// Can the count pass read its state rows faster through an LDS-DMA ring than with its plain loads?  
// One 12 GiB block of 848-byte rows (the state matrix at N = 833) is streamed once per launch in three forms:
//   1  read_bw.hip's contiguous plain loads: every lane 16 bytes, 8 loads in flight, 4 and 8 workgroups per CU
//   2  the count pass's pattern (store_cost.hip read pattern 1): 16 rows per instruction, four lanes x 16 bytes per row, all 14
//      loads of a half tile up front, a wave owns super-tiles of 32 rows, 2 workgroups per CU
//   3  global_load_lds_dwordx4, 1 KiB per instruction and lane-linear (every 128-byte line asked for once), into a ring of NS slots
//      of SR rows that belongs to the wave; the SAME wave waits on vmcnt and reads 16 rows back with ds_read_b128 in form 2's
//      (row, quad lane) order, then refills the slots it has read.  Default cache policy and nt; SR = 16 (13.25 KiB) and 8;
//      NS = 2..5; 4 and 8 waves per CU (workgroups of 4 waves; what does not fit the 160 KiB of LDS is left out).
// Every kernel xors the words it was asked to read (duplicates of the clamped last chunk masked out) into out[]: the three
// forms must agree, which checks the ring's slot and vmcnt arithmetic.  All forms run in one process, one launch each in
// turn, `reps` times after one unrecorded turn; printed per form: median, min, max in ms and the median's GB/s, then the
// verdict: the best form 3 against form 2, the difference of the medians over the larger of the two spreads (max - min).
// build: hipcc --offload-arch=gfx950 -O3 dma_stream.hip -o dma_stream       usage: dma_stream [reps=12] [matrix GiB=12]
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <functional>
#include <string>
#include <vector>
typedef unsigned int u32;
typedef u32 v4u __attribute__((ext_vector_type(4)));

constexpr long ROW = 848, TILE = 32 * ROW;
constexpr int CPR = 53;                                                                  // 16-byte chunks per row

__global__ void k_init(u32* p, long n) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) p[i] = (u32)i * 2654435761u ^ (u32)(i >> 32);
}

__device__ __forceinline__ void fold(u32 acc, long gw, u32* out) {                       // one atomic per wave, spread over 64 words
    for (int d = 32; d; d >>= 1) acc ^= __shfl_xor(acc, d);
    if ((threadIdx.x & 63) == 0) atomicXor(&out[gw & 63], acc);
}

// form 1
__global__ __launch_bounds__(256) void k_flat(const uint4* __restrict__ p, long n16, u32* out) {
    constexpr int U = 8;
    u32 acc = 0;
    const long stride = (long)gridDim.x * 256 * U;
    for (long i = (long)blockIdx.x * 256 * U + threadIdx.x; i < n16; i += stride) {
        uint4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = (i + 256L * u < n16) ? p[i + 256L * u] : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int u = 0; u < U; ++u) acc ^= v[u].x ^ v[u].y ^ v[u].z ^ v[u].w;
    }
    fold(acc, (long)blockIdx.x * 4 + (threadIdx.x >> 6), out);
}

// form 2
__global__ __launch_bounds__(256) void k_rows(const char* __restrict__ X, long nsuper, u32* out) {
    extern __shared__ char pad[];                                                        // (dynamic LDS sets the workgroups per CU)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u32 acc = 0;
    for (long st = (long)blockIdx.x * 4 + wave; st < nsuper; st += (long)gridDim.x * 4) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const char* rowp = X + (st * 32 + h * 16 + (lane >> 2)) * ROW;
            uint4 v[14];
#pragma unroll
            for (int i = 0; i < 14; ++i) {
                int c = 4 * i + (lane & 3);
                c = c < CPR - 1 ? c : CPR - 1;
                v[i] = *reinterpret_cast<const uint4*>(rowp + 16 * c);
            }
#pragma unroll
            for (int i = 0; i < 14; ++i) {
                const u32 x = v[i].x ^ v[i].y ^ v[i].z ^ v[i].w;
                acc ^= (i < 13 || (lane & 3) == 0) ? x : 0u;
            }
        }
    }
    fold(acc, (long)blockIdx.x * 4 + wave, out);
    if (acc == 0x12345678u && nsuper < 0) out[0] = pad[0];
}

// form 3.  Slot sequence number f of a wave: 16-row step t = f / Q (Q = 16 / SR slots per step), the wave's super-tile t >> 1,
// half t & 1.  NS slots are always in flight or unread; step t waits until all but the newest NS - Q have landed.
template <int SR, int NS, int AUX>
__global__ __launch_bounds__(256) void k_dma(const char* __restrict__ X, long nsuper, u32* out) {
    extern __shared__ __attribute__((aligned(16))) char ring[];
    constexpr int Q = 16 / SR, CH = SR * CPR, NI = (CH + 63) / 64, SLOT = SR * (int)ROW;
    static_assert(NS >= Q && (NS - Q) * NI <= 63, "ring shape");
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 3, b = lane >> 2;
    const long gw = (long)blockIdx.x * 4 + wave, TW = (long)gridDim.x * 4;
    if (gw >= nsuper) return;                                                            // (no barrier in this kernel)
    const long T = 2 * ((nsuper - gw + TW - 1) / TW);                                    // this wave's 16-row steps
    char* const my = ring + wave * (NS * SLOT);
    auto fill = [&](long f, int slot) {
        long t = f / Q;
        const int sub = (int)(f % Q);
        t = t < T ? t : T - 1;                                                           // past the end: the last step again, never read
        const char* src = X + ((gw + (t >> 1) * TW) * 32 + (t & 1) * 16 + sub * SR) * ROW + lane * 16;
        char* dst = my + slot * SLOT;
#pragma unroll
        for (int i = 0; i < NI; ++i)
            if (i < NI - 1 || lane < CH - (NI - 1) * 64)                                 // the slot's last piece is a partial one
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + i * 1024),
                                                 (__attribute__((address_space(3))) void*)(dst + i * 1024), 16, 0, AUX);
    };
#pragma unroll
    for (int s = 0; s < NS; ++s) fill(s, s);
    long f = NS;
    int rs = 0;
    u32 acc = 0;
    for (long t = 0; t < T; ++t) {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - Q) * NI) : "memory");
        const int rs1 = rs + 1 == NS ? 0 : rs + 1;
        const u32 s0 = (u32)(uintptr_t)(my + rs * SLOT), s1 = (u32)(uintptr_t)(my + rs1 * SLOT);
        const u32 a = (Q == 2 && b >= SR ? s1 : s0) + (u32)(b & (SR - 1)) * (u32)ROW + 16u * j;
        const u32 a13 = a - 16u * j + 16u * (CPR - 1);                                   // chunk 52 + j clamped to 52
        v4u v[14];
        asm volatile(
            "ds_read_b128 %0, %14\n\tds_read_b128 %1, %14 offset:64\n\tds_read_b128 %2, %14 offset:128\n\tds_read_b128 %3, %14 offset:192\n\t"
            "ds_read_b128 %4, %14 offset:256\n\tds_read_b128 %5, %14 offset:320\n\tds_read_b128 %6, %14 offset:384\n\tds_read_b128 %7, %14 offset:448\n\t"
            "ds_read_b128 %8, %14 offset:512\n\tds_read_b128 %9, %14 offset:576\n\tds_read_b128 %10, %14 offset:640\n\tds_read_b128 %11, %14 offset:704\n\t"
            "ds_read_b128 %12, %14 offset:768\n\tds_read_b128 %13, %15\n\ts_waitcnt lgkmcnt(0)"
            : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5]), "=&v"(v[6]), "=&v"(v[7]), "=&v"(v[8]), "=&v"(v[9]),
              "=&v"(v[10]), "=&v"(v[11]), "=&v"(v[12]), "=&v"(v[13])
            : "v"(a), "v"(a13)
            : "memory");
#pragma unroll
        for (int q = 0; q < Q; ++q) {                                                    // the slots just read are free: refill them
            fill(f++, rs);
            rs = rs + 1 == NS ? 0 : rs + 1;
        }
#pragma unroll
        for (int i = 0; i < 14; ++i) {
            const u32 x = v[i].x ^ v[i].y ^ v[i].z ^ v[i].w;
            acc ^= (i < 13 || j == 0) ? x : 0u;
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    fold(acc, gw, out);
}

struct Form {
    std::string name;
    bool dma;
    std::function<hipError_t()> launch;
    std::vector<float> ms;
    u32 sum;
};

template <int SR, int NS, int AUX>
static void add_dma(std::vector<Form>& forms, int waves_per_cu, int cus, const char* X, long nsuper, u32* out) {
    const int wgs = waves_per_cu / 4;
    const int need = 4 * NS * SR * (int)ROW, cap = 160 * 1024 / wgs, floor_ = 160 * 1024 / (wgs + 1) + 1024;
    char name[96];
    snprintf(name, sizeof name, "3 dma %-3s slot %2d rows x %d, %d waves/CU (%3d KiB LDS)", AUX ? "nt" : "def", SR, NS, waves_per_cu, wgs * need / 1024);
    if (need > cap) {
        printf("%s: does not fit\n", name);
        return;
    }
    const int shmem = std::max(need, floor_);                                            // no more than `wgs` workgroups on a CU
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_dma<SR, NS, AUX>), hipFuncAttributeMaxDynamicSharedMemorySize, shmem) != hipSuccess) {
        (void)hipGetLastError();
        printf("%s: %d bytes of LDS refused\n", name, shmem);
        return;
    }
    forms.push_back({name, true, [=] {
                         hipLaunchKernelGGL((k_dma<SR, NS, AUX>), dim3(cus * wgs), dim3(256), shmem, 0, X, nsuper, out);
                         return hipGetLastError();
                     }, {}, 0});
}

template <int AUX>
static void add_dma_sweep(std::vector<Form>& forms, int cus, const char* X, long nsuper, u32* out) {
    for (int w : {4, 8}) {
        add_dma<16, 2, AUX>(forms, w, cus, X, nsuper, out);
        add_dma<16, 3, AUX>(forms, w, cus, X, nsuper, out);
        add_dma<16, 4, AUX>(forms, w, cus, X, nsuper, out);
        add_dma<16, 5, AUX>(forms, w, cus, X, nsuper, out);
        add_dma<8, 2, AUX>(forms, w, cus, X, nsuper, out);
        add_dma<8, 3, AUX>(forms, w, cus, X, nsuper, out);
        add_dma<8, 4, AUX>(forms, w, cus, X, nsuper, out);
        add_dma<8, 5, AUX>(forms, w, cus, X, nsuper, out);
    }
}

int main(int argc, char** argv) {
    const int reps = argc > 1 ? atoi(argv[1]) : 12;
    const long XB = (argc > 2 ? atol(argv[2]) : 12L) << 30;
    const long nsuper = XB / TILE, bytes = nsuper * TILE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess) return 1;
    const int cus = prop.multiProcessorCount;
    char* X = nullptr;
    u32* out = nullptr;
    if (hipMalloc(&X, XB) != hipSuccess || hipMalloc(&out, 64 * 4) != hipSuccess) return 1;
    hipLaunchKernelGGL(k_init, dim3(cus * 8), dim3(256), 0, 0, reinterpret_cast<u32*>(X), XB / 4);
    if (hipDeviceSynchronize() != hipSuccess) return 1;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);

    std::vector<Form> forms;
    for (int bpc : {4, 8})
        forms.push_back({"1 flat plain loads x8, " + std::to_string(bpc) + " wg/CU", false, [=] {
                             hipLaunchKernelGGL(k_flat, dim3(cus * bpc), dim3(256), 0, 0, reinterpret_cast<const uint4*>(X), bytes / 16, out);
                             return hipGetLastError();
                         }, {}, 0});
    const int shmem2 = 160 * 1024 / 2 - 1024;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_rows), hipFuncAttributeMaxDynamicSharedMemorySize, shmem2);
    forms.push_back({"2 count-pass rows, 14 loads up front, 2 wg/CU", false, [=] {
                         hipLaunchKernelGGL(k_rows, dim3(cus * 2), dim3(256), shmem2, 0, X, nsuper, out);
                         return hipGetLastError();
                     }, {}, 0});
    const size_t form2 = forms.size() - 1;
    add_dma_sweep<0>(forms, cus, X, nsuper, out);
    add_dma_sweep<2>(forms, cus, X, nsuper, out);                                        // aux bit 1 = nt

    printf("%d CUs, %ld super-tiles of 32 rows x %ld bytes = %.3f GB per launch, %d recorded launches per form, in turn\n", cus, nsuper, ROW, bytes / 1e9, reps);
    for (int it = 0; it < reps + 1; ++it)
        for (Form& f : forms) {
            float ms = 0;
            (void)hipMemsetAsync(out, 0, 64 * 4, 0);
            (void)hipEventRecord(e0);
            const hipError_t err = f.launch();
            (void)hipEventRecord(e1);
            if (err != hipSuccess || hipEventSynchronize(e1) != hipSuccess) {            // nothing more on the GPU after a failure
                printf("%s: %s\n", f.name.c_str(), hipGetErrorString(err != hipSuccess ? err : hipGetLastError()));
                return 1;
            }
            (void)hipEventElapsedTime(&ms, e0, e1);
            if (it) f.ms.push_back(ms);
            u32 h[64], x = 0;
            (void)hipMemcpy(h, out, sizeof h, hipMemcpyDeviceToHost);
            for (u32 v : h) x ^= v;
            if (!it) f.sum = x;
            else if (x != f.sum) {
                printf("%s: checksum changed between launches (%08x, %08x)\n", f.name.c_str(), f.sum, x);
                return 1;
            }
        }

    bool agree = true;
    float med2 = 0, spread2 = 0, best = 1e9f, best_spread = 0;
    const Form* bestf = nullptr;
    for (size_t k = 0; k < forms.size(); ++k) {
        Form& f = forms[k];
        std::sort(f.ms.begin(), f.ms.end());
        const size_t n = f.ms.size();
        const float med = n & 1 ? f.ms[n / 2] : 0.5f * (f.ms[n / 2 - 1] + f.ms[n / 2]);
        printf("%-58s median %.3f ms  min %.3f  max %.3f  = %4.0f GB/s  xor %08x\n", f.name.c_str(), med, f.ms.front(), f.ms.back(), bytes / med / 1e6, f.sum);
        agree = agree && f.sum == forms[0].sum;
        if (k == form2) med2 = med, spread2 = f.ms.back() - f.ms.front();
        if (f.dma && med < best) best = med, best_spread = f.ms.back() - f.ms.front(), bestf = &f;
    }
    if (!agree) {
        printf("CHECKSUMS DIFFER: the timings above mean nothing\n");
        return 1;
    }
    if (bestf) {
        const float spread = std::max(spread2, best_spread);
        printf("best form 3: %s\nform 2 - best form 3 = %+.3f ms; larger spread %.3f ms; ratio %.2f (go needs > 3): %s\n", bestf->name.c_str(), med2 - best, spread,
               (med2 - best) / spread, med2 - best > 3 * spread ? "GO" : "NO-GO");
    }
    return 0;
}
