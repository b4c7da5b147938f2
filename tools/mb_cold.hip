// mb_cold.hip -- HBM ceilings of the K=3/M=10 encode's memory pattern from
// cold caches: 256 stripes x 1 MiB (bench.py's batched_1MiB layout,
// [stripe][block][row], rows of 349,696 bytes), launches rotated over buffer
// sets spanning > 768 MiB so no launch finds its bytes in the 256 MiB
// Infinity Cache.  Every variant moves the same bytes: 3 x 16-byte loads and
// 7 x 16-byte stores per lane per unit; the arithmetic is an XOR (a copy
// ceiling), except "prod", which is the production dispatcher's kernel.
//
// Walk variants:
//   lane     one 16-byte unit per lane, grid = units / 256 (production walk)
//   persist  persistent grid (CUs x 8 workgroups), grid-stride over units
//   xcd      as `lane`, but workgroups dealt so that the 8 XCDs (blockIdx % 8)
//            each sweep one contiguous eighth of the units
//   wave4    each wave owns 4 consecutive 1 KiB pieces of every block
//            (4 KiB contiguous per block per wave), lanes 1 KiB apart
//   plain    `lane` with default-policy stores instead of nt
//   ntload   `lane` with nt loads too
//   prod     the production dispatcher's kernel (launch_apply)
//   prod_bm  the production kernel on the same stripes stored block-major
//            (one long row per block, as fec_encode_batch collapses them)
// usage: tools/mb_cold.exe [buffer sets] [stripes] | tools/mb_cold.exe sweep | launch | blocks | tail | ldsweep | one
//   one      cfg2's stripe: the production kernel against the copy walk of the
//            register kernels' straight-line single-stripe form (mb_one)
// Ceilings: read3 (only the 3 loads), write7 (only the 7 stores), copy1
// (1 load, 1 store per unit).
//
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude tools/mb_cold.hip zfec_amd/csrc/bitslice.cpp \
//          zfec_amd/csrc/gf256.cpp zfec_amd/csrc/config.cpp zfec_amd/csrc/host_pool.cpp -ldl -lpthread \
//          -o tools/mb_cold.exe
#include "../zfec_amd/csrc/kernels.hip"

#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <string>
#include <vector>

using namespace zfec_hip;

#define CK(x)                                                                                  \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) {                                                                \
            fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            exit(1);                                                                           \
        }                                                                                      \
    } while (0)

namespace {

constexpr int K = 3, R = 7;

struct Lay {
    uint8_t* in;
    uint8_t* out;
    uint64_t ld;       // row bytes
    uint32_t cps;      // 16-byte chunks per row
    uint32_t units;    // cps * nstripes
};

__device__ __forceinline__ void unit_io(const Lay& L, uint32_t u, bool ntload, bool ntstore, int mode) {
    const uint32_t s = u / L.cps, c = u - s * L.cps;
    const uint64_t ib = uint64_t(s) * K * L.ld + uint64_t(c) * 16;
    const uint64_t ob = uint64_t(s) * R * L.ld + uint64_t(c) * 16;
    u32x4 acc = {0u, 0u, 0u, 0u};
    if (mode != 2) {  // loads
        const int nl = mode == 3 ? 1 : K;
        for (int j = 0; j < nl; ++j) {
            const u32x4* p = reinterpret_cast<const u32x4*>(L.in + ib + j * L.ld);
            acc ^= ntload ? __builtin_nontemporal_load(p) : *p;
        }
    } else {
        acc = u32x4{u, u + 1, u + 2, u + 3};
    }
    if (mode == 1) {  // read only: keep the loads alive
        if (acc.x == 0x12345678u && acc.y == 0x9abcdef0u) *reinterpret_cast<u32x4*>(L.out + ob) = acc;
        return;
    }
    const int ns = mode == 3 ? 1 : R;
    for (int r = 0; r < ns; ++r) {
        u32x4* q = reinterpret_cast<u32x4*>(L.out + ob + r * L.ld);
        if (ntstore)
            __builtin_nontemporal_store(acc ^ uint32_t(r), q);
        else
            *q = acc ^ uint32_t(r);
    }
}

// walk: 0 lane, 1 persist, 2 xcd, 3 wave4.  mode: 0 encode-shaped, 1 read3, 2 write7, 3 copy1
template <int WALK, bool NTL, bool NTS, int MODE>
__global__ __launch_bounds__(256) void mb(const Lay L) {
    if constexpr (WALK == 0) {
        const uint32_t u = blockIdx.x * 256 + threadIdx.x;
        if (u < L.units) unit_io(L, u, NTL, NTS, MODE);
    } else if constexpr (WALK == 1) {
        for (uint32_t u = blockIdx.x * 256 + threadIdx.x; u < L.units; u += gridDim.x * 256)
            unit_io(L, u, NTL, NTS, MODE);
    } else if constexpr (WALK == 2) {
        const uint32_t nwg = gridDim.x, q = nwg / 8, rr = nwg % 8, x = blockIdx.x % 8;
        const uint32_t wg = (x < rr ? x * (q + 1) : rr * (q + 1) + (x - rr) * q) + blockIdx.x / 8;
        const uint32_t u = wg * 256 + threadIdx.x;
        if (u < L.units) unit_io(L, u, NTL, NTS, MODE);
    } else {
        // wave w of the grid owns 64-lane pieces 4w..4w+3 of the unit sequence
        const uint32_t wave = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
        for (int p = 0; p < 4; ++p) {
            const uint32_t u = (wave * 4 + p) * 64 + lane;
            if (u < L.units) unit_io(L, u, NTL, NTS, MODE);
        }
    }
}

// Encode-shaped copy walk (`lane`) whose last workgroups store with a
// write-through policy (SP: 1 sc1, 2 sc0 sc1, 3 nt sc1) and the rest with nt:
// does the end-of-kernel write-back of dirty L2 lines set part of the fixed
// per-launch cost?  Workgroups >= tail_wg take the write-through stores.
template <int SP>
__device__ __forceinline__ void store_wt(uint8_t* p, u32x4 v) {
    if constexpr (SP == 1)
        asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
    else if constexpr (SP == 2)
        asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
    else
        store16_pol<3>(p, v);
}

template <int SP>
__global__ __launch_bounds__(256) void mb_tail(const Lay L, uint32_t tail_wg) {
    const uint32_t u = blockIdx.x * 256 + threadIdx.x;
    if (u >= L.units) return;
    const uint32_t s = u / L.cps, c = u - s * L.cps;
    const uint64_t ib = uint64_t(s) * K * L.ld + uint64_t(c) * 16;
    const uint64_t ob = uint64_t(s) * R * L.ld + uint64_t(c) * 16;
    u32x4 acc = {0u, 0u, 0u, 0u};
    for (int j = 0; j < K; ++j) acc ^= *reinterpret_cast<const u32x4*>(L.in + ib + j * L.ld);
    const bool wt = blockIdx.x >= tail_wg;
    for (int r = 0; r < R; ++r) {
        uint8_t* q = L.out + ob + r * L.ld;
        if (wt)
            store_wt<SP>(q, acc ^ uint32_t(r));
        else
            __builtin_nontemporal_store(acc ^ uint32_t(r), reinterpret_cast<u32x4*>(q));
    }
}

template <int SP>
float run_tail(const std::vector<Lay>& sets, int reps, uint32_t grid, uint32_t tail_wg) {
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    for (int i = 0; i < 3; ++i) hipLaunchKernelGGL(mb_tail<SP>, dim3(grid), dim3(256), 0, 0, sets[i % sets.size()], tail_wg);
    CK(hipEventRecord(a, 0));
    for (int i = 0; i < reps; ++i)
        hipLaunchKernelGGL(mb_tail<SP>, dim3(grid), dim3(256), 0, 0, sets[(i + 3) % sets.size()], tail_wg);
    CK(hipEventRecord(b, 0));
    CK(hipEventSynchronize(b));
    float ms = 0;
    CK(hipEventElapsedTime(&ms, a, b));
    return ms / reps;
}

template <int WALK, bool NTL, bool NTS, int MODE>
float run(const std::vector<Lay>& sets, int reps, uint32_t grid) {
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    for (int i = 0; i < 3; ++i) hipLaunchKernelGGL((mb<WALK, NTL, NTS, MODE>), dim3(grid), dim3(256), 0, 0, sets[i % sets.size()]);
    CK(hipEventRecord(a, 0));
    for (int i = 0; i < reps; ++i)
        hipLaunchKernelGGL((mb<WALK, NTL, NTS, MODE>), dim3(grid), dim3(256), 0, 0, sets[(i + 3) % sets.size()]);
    CK(hipEventRecord(b, 0));
    CK(hipEventSynchronize(b));
    float ms = 0;
    CK(hipEventElapsedTime(&ms, a, b));
    return ms / reps;
}

// One production launch (launch_apply) of the K=3/M=10 encode rows over a buffer set.
struct Prod {
    const uint8_t* in[K];
    uint8_t* out[R];
    ApplySpec a;
};
static const uint8_t kCoef[R * K] = {15, 8, 6, 45, 48, 28, 153, 224, 120, 11, 231, 237, 137, 59, 179, 70, 241, 182, 186, 217, 98};

void fill_prod(Prod& p, const Lay& L, uint64_t row, uint64_t sz, uint64_t ns, uint64_t in_ss, uint64_t out_ss) {
    for (int q = 0; q < K; ++q) p.in[q] = L.in + q * row;
    for (int q = 0; q < R; ++q) p.out[q] = L.out + q * row;
    p.a = ApplySpec{kCoef, K, K, R, p.in, p.out, sz, ns, in_ss, out_ss, false};
}

float time_prod(std::vector<Prod>& jobs, int reps) {
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    for (int i = 0; i < 3; ++i) CK(launch_apply(jobs[i % jobs.size()].a, 0));
    CK(hipEventRecord(a, 0));
    for (int i = 0; i < reps; ++i) CK(launch_apply(jobs[(i + 3) % jobs.size()].a, 0));
    CK(hipEventRecord(b, 0));
    CK(hipEventSynchronize(b));
    float ms = 0;
    CK(hipEventElapsedTime(&ms, a, b));
    return ms / reps;
}

float run_prod(const std::vector<Lay>& sets, int reps, uint64_t sz, uint32_t ns) {
    std::vector<Prod> jobs(sets.size());
    for (size_t i = 0; i < sets.size(); ++i) fill_prod(jobs[i], sets[i], sets[i].ld, sz, ns, K * sets[i].ld, R * sets[i].ld);
    return time_prod(jobs, reps);
}

// The same stripes stored block-major (block j of every stripe back to back:
// one row of ns * sz bytes per block), as fec_encode_batch collapses them:
// one launch over 10 long streams.
float run_prod_bm(const std::vector<Lay>& sets, int reps, uint64_t sz, uint32_t ns) {
    std::vector<Prod> jobs(sets.size());
    for (size_t i = 0; i < sets.size(); ++i) fill_prod(jobs[i], sets[i], sz * ns, sz * ns, 1, 0, 0);
    return time_prod(jobs, reps);
}

}  // namespace

// Size sweep of the production kernel on one long stripe per block (block-major),
// cold: how the HBM fraction of a K=3/M=10 encode grows with the launch's size.
int sweep() {
    const uint64_t sz1 = (1u << 20) / 3 + 1;
    for (uint32_t ns : {16u, 32u, 64u, 128u, 256u, 512u, 1024u}) {
        const uint64_t fp = uint64_t(K + R) * sz1 * ns;
        const int nsets = std::max<int>(2, int((1536ull << 20) / fp) + 1);
        std::vector<Lay> sets(nsets);
        for (auto& L : sets) {
            CK(hipMalloc(&L.in, ns * K * sz1));
            CK(hipMalloc(&L.out, ns * R * sz1));
            CK(hipMemset(L.in, 0x5A, ns * K * sz1));
            L.ld = sz1;
        }
        CK(hipDeviceSynchronize());
        float best = 1e9f, sum = 0.f;
        for (int rnd = 0; rnd < 3; ++rnd) {
            const float ms = run_prod_bm(sets, 20, sz1, ns);
            best = std::min(best, ms);
            sum += ms;
        }
        const double bytes = double(K + R) * sz1 * ns;
        printf("sweep ns=%4u  %8.1f MB/launch  %8.1f us  %7.1f GB/s  (%.3f of 8 TB/s) mean-of-3 %.1f us  sets=%d\n", ns,
               bytes / 1e6, best * 1e3, bytes / (best * 1e-3) / 1e9, bytes / (best * 1e-3) / 8e12, sum / 3 * 1e3, nsets);
        for (auto& L : sets) {
            CK(hipFree(L.in));
            CK(hipFree(L.out));
        }
    }
    return 0;
}

// Row-stride sweep of the production kernel on 256 object-major 1 MiB stripes
// (rows of sz = 349,526 bytes at stride ld): does the HBM fraction depend on
// where the 10 rows of a stripe fall relative to each other?
int ldsweep() {
    const uint32_t ns = 256;
    const uint64_t sz = (1u << 20) / 3 + 1;
    const uint64_t lds[] = {349696, 349696 + 128, 349696 + 512, 349696 + 2048, 352256, 352256 + 4096,
                            356352 + 8192, 393216, 1u << 19, (1u << 19) + 4096};
    for (int rnd = 0; rnd < 2; ++rnd)
        for (uint64_t ld : lds) {
            const uint64_t fp = uint64_t(K + R) * ld * ns;
            const int nsets = std::max<int>(2, int((1536ull << 20) / fp) + 1);
            std::vector<Lay> sets(nsets);
            for (auto& L : sets) {
                CK(hipMalloc(&L.in, ns * K * ld));
                CK(hipMalloc(&L.out, ns * R * ld));
                CK(hipMemset(L.in, 0x5A, ns * K * ld));
                L.ld = ld;
            }
            CK(hipDeviceSynchronize());
            const float ms = run_prod(sets, 20, sz, ns);
            const double bytes = double(K + R) * sz * ns;
            printf("ldsweep ld=%8llu (ld %% 4096 = %4llu)  %8.1f us  %7.1f GB/s  (%.3f of 8 TB/s)  sets=%d\n",
                   (unsigned long long)ld, (unsigned long long)(ld % 4096), ms * 1e3, bytes / (ms * 1e-3) / 1e9,
                   bytes / (ms * 1e-3) / 8e12, nsets);
            for (auto& L : sets) {
                CK(hipFree(L.in));
                CK(hipFree(L.out));
            }
        }
    return 0;
}

// cfg2's shape (one 64 MiB K=3/M=10 stripe: 3 + 7 rows of 22,369,792 bytes),
// cold rotation: the nt copy walk with its last fraction f of workgroups
// storing write-through, against the production kernel.
int tail() {
    const uint64_t sz = (64ull << 20) / 3 + 1, ld = (sz + 255) / 256 * 256;
    const int nsets = int((1536ull << 20) / (10 * ld)) + 1;
    std::vector<Lay> sets(nsets);
    for (auto& L : sets) {
        CK(hipMalloc(&L.in, K * ld));
        CK(hipMalloc(&L.out, R * ld));
        CK(hipMemset(L.in, 0x5A, K * ld));
        CK(hipMemset(L.out, 0, R * ld));
        L.ld = ld;
        L.cps = static_cast<uint32_t>(ld / 16);
        L.units = L.cps;
    }
    CK(hipDeviceSynchronize());
    const uint32_t grid = (sets[0].units + 255) / 256;
    const double bytes = double(K + R) * ld;
    auto rep = [&](const char* name, float ms) {
        printf("tail %-24s %7.2f us  %7.1f GB/s  (%.3f of 8 TB/s)  sets=%d\n", name, ms * 1e3,
               bytes / (ms * 1e-3) / 1e9, bytes / (ms * 1e-3) / 8e12, nsets);
    };
    for (int rnd = 0; rnd < 3; ++rnd) {
        printf("-- round %d\n", rnd);
        rep("prod", run_prod(sets, 40, sz, 1));
        for (double f : {0.0, 0.02, 0.05, 0.1, 0.2, 1.0}) {
            const uint32_t tw = grid - static_cast<uint32_t>(f * grid);
            char nm[64];
            snprintf(nm, sizeof nm, "f=%.2f sc0sc1", f);
            rep(nm, run_tail<2>(sets, 40, grid, tw));
            snprintf(nm, sizeof nm, "f=%.2f ntsc1", f);
            rep(nm, run_tail<3>(sets, 40, grid, tw));
            snprintf(nm, sizeof nm, "f=%.2f sc1", f);
            rep(nm, run_tail<1>(sets, 40, grid, tw));
        }
    }
    return 0;
}

// The walk of the register kernels' single-stripe form (kernels.hip
// reg_body_one) with the arithmetic replaced by an XOR: the lane's unit is its
// global index, the last chunk and the spare lanes of the last workgroup are
// shifted back to end at the row's end, no division, no branch, nt sc1 stores.
// `one` times it against the dividing lane walk with the same stores (mb_tail,
// f = 1) and the production kernel on cfg2's stripe, cold, interleaved.
__global__ __launch_bounds__(256) void mb_one(const Lay L) {
    const uint64_t sz = L.ld;
    const uint64_t own = static_cast<uint64_t>(blockIdx.x * 256 + threadIdx.x) * 16;
    const uint64_t off = own + 16 <= sz ? own : sz - 16;
    u32x4 acc = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < K; ++j) acc ^= load16(L.in + off + j * L.ld);
#pragma unroll
    for (int r = 0; r < R; ++r) store16_pol<3>(L.out + off + r * L.ld, acc ^ uint32_t(r));
}

float run_one(const std::vector<Lay>& sets, int reps, uint32_t grid) {
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    for (int i = 0; i < 3; ++i) hipLaunchKernelGGL(mb_one, dim3(grid), dim3(256), 0, 0, sets[i % sets.size()]);
    CK(hipEventRecord(a, 0));
    for (int i = 0; i < reps; ++i) hipLaunchKernelGGL(mb_one, dim3(grid), dim3(256), 0, 0, sets[(i + 3) % sets.size()]);
    CK(hipEventRecord(b, 0));
    CK(hipEventSynchronize(b));
    float ms = 0;
    CK(hipEventElapsedTime(&ms, a, b));
    return ms / reps;
}

int one() {
    const uint64_t sz = (64ull << 20) / 3 + 1, ld = (sz + 255) / 256 * 256;
    const int nsets = int((1536ull << 20) / (10 * ld)) + 1;
    std::vector<Lay> sets(nsets);
    for (auto& L : sets) {
        CK(hipMalloc(&L.in, K * ld));
        CK(hipMalloc(&L.out, R * ld));
        CK(hipMemset(L.in, 0x5A, K * ld));
        CK(hipMemset(L.out, 0, R * ld));
        L.ld = ld;
        L.cps = static_cast<uint32_t>(ld / 16);
        L.units = L.cps;
    }
    CK(hipDeviceSynchronize());
    const uint32_t grid = (sets[0].units + 255) / 256;
    const double bytes = double(K + R) * ld;
    for (int rnd = 0; rnd < 5; ++rnd) {
        const float prod = run_prod(sets, 40, ld, 1), walk = run_tail<3>(sets, 40, grid, 0), str8 = run_one(sets, 40, grid);
        printf("one round %d  prod %6.2f us (%.3f of 8 TB/s)  copy, dividing walk %6.2f us  copy, straight-line %6.2f us  "
               "prod = %.3f of the straight-line copy\n",
               rnd, prod * 1e3, bytes / (prod * 1e-3) / 8e12, walk * 1e3, str8 * 1e3, str8 / prod);
    }
    return 0;
}

// The `lane` copy walk with BS-thread workgroups (256 in production): fewer,
// larger workgroups cost less to dispatch (launch_cost) -- does the walk gain?
template <int BS>
__global__ __launch_bounds__(BS) void mb_bs(const Lay L) {
    const uint32_t u = blockIdx.x * BS + threadIdx.x;
    if (u < L.units) unit_io(L, u, false, true, 0);
}

template <int BS>
float run_bs(const std::vector<Lay>& sets, int reps) {
    const uint32_t grid = (sets[0].units + BS - 1) / BS;
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    for (int i = 0; i < 3; ++i) hipLaunchKernelGGL(mb_bs<BS>, dim3(grid), dim3(BS), 0, 0, sets[i % sets.size()]);
    CK(hipEventRecord(a, 0));
    for (int i = 0; i < reps; ++i) hipLaunchKernelGGL(mb_bs<BS>, dim3(grid), dim3(BS), 0, 0, sets[(i + 3) % sets.size()]);
    CK(hipEventRecord(b, 0));
    CK(hipEventSynchronize(b));
    float ms = 0;
    CK(hipEventElapsedTime(&ms, a, b));
    return ms / reps;
}

// 256 object-major 1 MiB stripes (as main) and the cfg2 stripe, cold: the
// copy walk at 256 / 512 / 1024 threads per workgroup.
int blocks() {
    for (int shape = 0; shape < 2; ++shape) {
        const uint32_t ns = shape == 0 ? 256 : 1;
        const uint64_t sz = shape == 0 ? (1u << 20) / 3 + 1 : (64ull << 20) / 3 + 1;
        const uint64_t ld = (sz + 255) / 256 * 256;
        const int nsets = std::max<int>(2, int((1536ull << 20) / (10 * ld * ns)) + 1);
        std::vector<Lay> sets(nsets);
        for (auto& L : sets) {
            CK(hipMalloc(&L.in, ns * K * ld));
            CK(hipMalloc(&L.out, ns * R * ld));
            CK(hipMemset(L.in, 0x5A, ns * K * ld));
            L.ld = ld;
            L.cps = static_cast<uint32_t>(ld / 16);
            L.units = L.cps * ns;
        }
        CK(hipDeviceSynchronize());
        const double bytes = double(K + R) * ld * ns;
        for (int rnd = 0; rnd < 3; ++rnd) {
            const float t256 = run_bs<256>(sets, 20), t512 = run_bs<512>(sets, 20), t1024 = run_bs<1024>(sets, 20);
            printf("blocks %s  256: %7.2f us (%.3f)  512: %7.2f us (%.3f)  1024: %7.2f us (%.3f)\n",
                   shape == 0 ? "256 x 1 MiB object-major" : "cfg2 64 MiB stripe      ", t256 * 1e3,
                   bytes / (t256 * 1e-3) / 8e12, t512 * 1e3, bytes / (t512 * 1e-3) / 8e12, t1024 * 1e3,
                   bytes / (t1024 * 1e-3) / 8e12);
        }
        for (auto& L : sets) {
            CK(hipFree(L.in));
            CK(hipFree(L.out));
        }
    }
    return 0;
}

// Fixed cost of a launch: back-to-back launches of a kernel that does no
// memory work, with one workgroup and with the cfg2 encode's grid (one
// 16-byte unit per lane of a 22,369,792-byte row: 5,462 workgroups of 256).
__global__ __launch_bounds__(256) void mb_empty(uint32_t* out, uint32_t v) {
    if (v == 0x12345678u && threadIdx.x == 0) out[blockIdx.x] = v;
}

int launch_cost() {
    uint32_t* out;
    CK(hipMalloc(&out, 1 << 20));
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    for (uint32_t grid : {1u, 256u, 5462u, 21845u, 87381u}) {
        for (int i = 0; i < 10; ++i) hipLaunchKernelGGL(mb_empty, dim3(grid), dim3(256), 0, 0, out, 1u);
        CK(hipDeviceSynchronize());
        CK(hipEventRecord(a, 0));
        for (int i = 0; i < 200; ++i) hipLaunchKernelGGL(mb_empty, dim3(grid), dim3(256), 0, 0, out, 1u);
        CK(hipEventRecord(b, 0));
        CK(hipEventSynchronize(b));
        float ms = 0;
        CK(hipEventElapsedTime(&ms, a, b));
        printf("launch grid=%6u x 256  %6.2f us per launch (back to back, empty kernel)\n", grid, ms * 1e3 / 200);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "sweep") return sweep();
    if (argc > 1 && std::string(argv[1]) == "launch") return launch_cost();
    if (argc > 1 && std::string(argv[1]) == "blocks") return blocks();
    if (argc > 1 && std::string(argv[1]) == "tail") return tail();
    if (argc > 1 && std::string(argv[1]) == "one") return one();
    if (argc > 1 && std::string(argv[1]) == "ldsweep") return ldsweep();
    const uint32_t ns = argc > 2 ? atoi(argv[2]) : 256;
    const uint64_t sz = (1u << 20) / 3 + 1;  // 349,526
    const uint64_t ld = (sz + 255) / 256 * 256;
    const int nsets = argc > 1 ? atoi(argv[1]) : 2;
    const int reps = 20;
    std::vector<Lay> sets(nsets);
    for (auto& L : sets) {
        CK(hipMalloc(&L.in, ns * K * ld));
        CK(hipMalloc(&L.out, ns * R * ld));
        CK(hipMemset(L.in, 0x5A, ns * K * ld));
        CK(hipMemset(L.out, 0, ns * R * ld));
        L.ld = ld;
        L.cps = static_cast<uint32_t>(ld / 16);
        L.units = L.cps * ns;
    }
    CK(hipDeviceSynchronize());
    int ncu = 256;
    hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, 0);
    const uint32_t units = sets[0].units;
    const uint32_t g_lane = (units + 255) / 256, g_persist = ncu * 8, g_wave4 = (units + 1023) / 1024;
    const double enc_bytes = double(K + R) * ld * ns;
    auto rep = [&](const char* name, float ms, double bytes) {
        printf("%-10s %8.1f us  %7.1f GB/s  (%.3f of 8 TB/s)  sets=%d\n", name, ms * 1e3, bytes / (ms * 1e-3) / 1e9,
               bytes / (ms * 1e-3) / 8e12, nsets);
    };
    for (int round = 0; round < 3; ++round) {
        printf("-- round %d\n", round);
        rep("prod", run_prod(sets, reps, sz, ns), double(K + R) * sz * ns);
        rep("prod_bm", run_prod_bm(sets, reps, sz, ns), double(K + R) * sz * ns);
        rep("lane", run<0, false, true, 0>(sets, reps, g_lane), enc_bytes);
        rep("persist", run<1, false, true, 0>(sets, reps, g_persist), enc_bytes);
        rep("xcd", run<2, false, true, 0>(sets, reps, g_lane), enc_bytes);
        rep("wave4", run<3, false, true, 0>(sets, reps, g_wave4), enc_bytes);
        rep("plain", run<0, false, false, 0>(sets, reps, g_lane), enc_bytes);
        rep("ntload", run<0, true, true, 0>(sets, reps, g_lane), enc_bytes);
        rep("read3", run<0, false, true, 1>(sets, reps, g_lane), double(K) * ld * ns);
        rep("write7", run<0, false, true, 2>(sets, reps, g_lane), double(R) * ld * ns);
        rep("copy1", run<0, false, true, 3>(sets, reps, g_lane), 2.0 * ld * ns);
        rep("copy1_pl", run<0, false, false, 3>(sets, reps, g_lane), 2.0 * ld * ns);
    }
    return 0;
}
