// kernels.hip -- GF(2^8) matrix-apply kernels for gfx950 (MI355X, CDNA4).
//
// The hot loop of zfec is _addmul1 (zfec/fec.c:170-204): dst[i] ^= c*src[i]
// through a 256-byte table row per coefficient, driven by fec_encode
// (fec.c:487-505) and fec_decode (fec.c:527-557).  Here one kernel reads each
// input chunk from HBM once and produces every requested output from it:
//
//   * each lane owns a 16-byte (or 8-byte) column slice of every block, so a
//     wave's loads and stores are 1 KiB (512 B) contiguous;
//   * multiplication by a constant c is GF(2)-linear, so
//       c*x = T0[x & 7] ^ T1[(x >> 3) & 7] ^ T2[x >> 6]
//     with three 8/8/4-entry byte tables; v_perm_b32 looks up four bytes at
//     once in an 8-byte table held in a register pair;
//   * partial products are merged by v_bitop3_b32 (gfx950's 3-input logic
//     op; truth table 0x96 = XOR3).
//
// Kernel families:
//   matapply_reg<K, R>  compile-time k <= 4 and r <= 8 (encode K=3/M=10 is
//                       <3,7>, its decode <3,3>): all K*R tables arrive in a
//                       kernel argument block sized to them (RegJob) and stay
//                       in registers; the per-chunk body is straight-line code.
//   matapply_rows<K, R> the same arithmetic, one wave per stripe of short blocks.
//   matapply_mixed<K>   the same arithmetic, K outputs, each stripe's tables picked
//                       by its pattern id from a device-side table (scalar loads).
//   ragged_walk         not a kernel: the walk of the six ragged families below,
//                       every stripe its own size.  A wave walks a short range of
//                       1 KiB units, finds its stripe by a search over their prefix
//                       sum (ragged_scan writes it for device-side sizes) and reads
//                       each stripe's descriptor by scalar loads.
//   matapply_ragged<K, R> matapply_reg's arithmetic per unit of the walk
//                       (fec_encode_batch_ragged / fec_decode_batch_ragged).
//   matverify_reg<K, R> the same arithmetic, nothing stored: the R rows are compared
//                       with the stored check blocks and only mismatch bits are
//                       OR-ed out (fec_verify_batch); rows_differ compares rows
//                       another kernel computed, for the shapes past k = 4.
//   matlocate_reg<K, R> matverify_reg with the R syndromes kept in registers: waves
//                       that saw a nonzero one test which single basis block
//                       explains them (fec_locate_batch); rows_locate does the
//                       same past k = 4 or 8 checks, locate_finish turns each
//                       stripe's bits into its verdict.
//   matverify_ragged<K, R>, matlocate_ragged<K, R>
//                       those two units inside ragged_walk: the bits of
//                       a stripe are gathered per wave and OR-ed out once, and
//                       ragged_unfit marks the stripes a device-side descriptor
//                       put outside the arena (fec_verify_batch_ragged /
//                       fec_locate_batch_ragged).
//   pairs_locate        over the stripes locate2_finish listed as MANY: the c
//                       syndromes in LDS, every pair of slots tested against
//                       them (fec_locate2_batch); pairs_finish names the one
//                       pair left, pairs_correct rewrites it (fec_correct2_batch).
//   pairs_locate_ragged, pairs_correct_ragged
//                       the same two units over the dirty list of a ragged
//                       location, each listed stripe's size and offset read by
//                       scalar loads (fec_locate2_batch_ragged /
//                       fec_correct2_batch_ragged).
//   matrepair_mixed<K, R> matapply_mixed with R rows per pattern instead of K, each
//                       row stored only where its pattern's live-row mask says
//                       so (fec_repair_batch).
//   matupdate_reg<C, R> matrepair_mixed's shape with one record per primary: the C
//                       changed blocks of a stripe (deltas, or old and new
//                       bytes) XOR-ed into R stored rows in place, for any k
//                       (fec_update_batch).  Blocks end with the byte tail.
//   matrepair_ragged<K, R>, matcorrect_ragged<K>
//                       ragged_walk around matrepair_mixed's per-stripe record (a
//                       size AND a pattern per stripe) and around matcorrect_reg's
//                       unit, the stripe's verdict read with its descriptor
//                       (fec_repair_batch_ragged / fec_correct_batch_ragged).
//   matupdate_ragged<C, R> matupdate_reg's wave step inside ragged_walk, any k: the
//                       one ragged kernel that XORs into its output, so its
//                       blocks end with the byte tail (fec_update_batch_ragged).
//   matapply_lds        any k <= 32, r <= 48 (longer codes are split by the
//                       caller): each workgroup expands its coefficients into
//                       LDS tables from a compile-time bank of all 256 values;
//                       rows in register tiles, inputs in prefetched groups.
//   matapply_bsr<RT>    bit-sliced, coefficients as run-time data, any
//                       k <= 256, r <= 256: one call per coefficient into
//                       precompiled multiply-by-constant routines
//                       (gf_routines.inc); past 32 inputs or 40 rows its
//                       pointers and coefficients come from a device-side table.
//   matapply_bsr<RT,mix> matapply_bsr for 4 < k <= 32 with a pattern id per stripe:
//                       the id picks the record (routine addresses, live-row
//                       mask) its unit walks with (fec_decode_batch_mixed,
//                       fec_repair_batch, fec_repair_batch_planned).
//   matverify_bsr<RT>   matapply_bsr's walk for 4 < k <= 32 with the rows kept as
//                       bit-planes and compared with the stored check blocks
//                       instead of stored: fec_verify_batch on wide codes reads
//                       every block once and needs no scratch.
//   matapply_bsg        bit-sliced, coefficients as run-time data, k <= 256
//                       (past 32 inputs its pointers and coefficients come
//                       from a device-side table).
//   matapply_small      launches too small to fill the chip, wide codes.
//
// Measured issue rates on gfx950 (tools/mb_valu.hip): v_perm_b32 and
// v_bitop3_b32 (VOP3) sustain ~37 T lane-ops/s chip-wide, plain VOP2 ops
// ~60 T.  A coefficient costs 3 v_perm + 1.5 v_bitop3 per 4 bytes, so K=3/M=10
// (~9 VOP3 per input byte, ~22 T ops/s at the HBM roofline) is memory-bound,
// while wide codes are bound by VALU issue (K=20/M=60: 45 VOP3 per input
// byte, <= ~0.8 TB/s of input).
#include "kernels.hpp"

#include <hip/hip_runtime.h>

#include "bitslice.hpp"
#include "config.hpp"

#include <array>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <unordered_map>
#include <vector>
#include <type_traits>
#include <utility>

namespace zfec_hip {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}

// v_perm_b32: byte i of the result = byte sel_i of the 8-byte value {hi:lo}
// (selector 0-3 -> lo, 4-7 -> hi).
__device__ __forceinline__ uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel) {
    return __builtin_amdgcn_perm(hi, lo, sel);
}

// ---- tables -----------------------------------------------------------------
// For a coefficient c, five dwords:
//   w0/w1 = c*{0..7}             (indexed by bits 0-2 of x)
//   w2/w3 = c*{0,8,...,56}       (bits 3-5)
//   w4    = c*{0,64,128,192}     (bits 6-7)
// All 256 values are built at compile time into constant memory (8 dwords
// per value, 8 KiB).

struct TableBank {
    uint32_t w[256 * 8];
};

constexpr uint32_t ct_xtime(uint32_t v) { return ((v << 1) & 0x100u) ? (((v << 1) ^ 0x11Du) & 0xFFu) : (v << 1); }

constexpr TableBank make_bank() {
    TableBank b{};
    for (uint32_t c = 0; c < 256; ++c) {
        uint32_t p[8] = {};
        p[0] = c;  // p[i] = c * alpha^i = c * 2^i
        for (int i = 1; i < 8; ++i) p[i] = ct_xtime(p[i - 1]);
        for (int h = 0; h < 2; ++h) {
            uint32_t lo = 0, hi = 0;
            for (int n = 0; n < 8; ++n) {
                const uint32_t e =
                    ((n & 1) ? p[3 * h] : 0u) ^ ((n & 2) ? p[3 * h + 1] : 0u) ^ ((n & 4) ? p[3 * h + 2] : 0u);
                if (n < 4)
                    lo |= e << (8 * n);
                else
                    hi |= e << (8 * (n - 4));
            }
            b.w[c * 8 + 2 * h] = lo;
            b.w[c * 8 + 2 * h + 1] = hi;
        }
        b.w[c * 8 + 4] = (p[6] << 8) | (p[7] << 16) | ((p[6] ^ p[7]) << 24);
    }
    return b;
}

__constant__ TableBank g_bank = make_bank();

// Host copy of the bank: the register kernels get their coefficients'
// tables in the kernel arguments.
constexpr TableBank kHostBank = make_bank();

// dst[0..5) = the table of coefficient `coef`.
inline void host_tab(uint32_t* dst, uint8_t coef) {
    std::memcpy(dst, &kHostBank.w[uint32_t(coef) * 8], 5 * sizeof(uint32_t));
}

struct Tab {
    uint32_t w0, w1, w2, w3, w4;
};

// ---- arithmetic ---------------------------------------------------------------

struct Sel {
    uint32_t s0, s1, s2;
};

__device__ __forceinline__ Sel selectors(uint32_t x) {
    return Sel{x & 0x07070707u, (x >> 3) & 0x07070707u, (x >> 6) & 0x03030303u};
}

// sum_j c_j*x_j for four bytes of one output row: the 3K partial products are
// merged by a chain of XOR3s, 3K v_perm + ceil((3K-1)/2) v_bitop3.
template <int K>
__device__ __forceinline__ uint32_t gf_dot(const Tab (&T)[K], const Sel (&s)[K]) {
    uint32_t p[3 * K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        p[3 * j + 0] = perm(T[j].w1, T[j].w0, s[j].s0);
        p[3 * j + 1] = perm(T[j].w3, T[j].w2, s[j].s1);
        p[3 * j + 2] = perm(T[j].w4, T[j].w4, s[j].s2);
    }
    uint32_t acc = xor3(p[0], p[1], p[2]);
#pragma unroll
    for (int i = 3; i + 1 < 3 * K; i += 2) acc = xor3(acc, p[i], p[i + 1]);
    if constexpr ((3 * K) % 2 == 0) acc ^= p[3 * K - 1];
    return acc;
}

// ---- memory -------------------------------------------------------------------

__device__ __forceinline__ u32x4 load16(const uint8_t* p) {
    u32x4 v;
    __builtin_memcpy(&v, p, 16);  // global_load_dwordx4; unaligned addresses are legal on gfx950
    return v;
}

__device__ __forceinline__ void store16(uint8_t* p, u32x4 v) { __builtin_memcpy(p, &v, 16); }

// Streaming store (global_store_dwordx4 ... nt): outputs are written once and
// not re-read by this kernel.
template <bool NT>
__device__ __forceinline__ void store16_out(uint8_t* p, u32x4 v) {
    if constexpr (NT)
        __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p));
    else
        store16(p, v);
}

// Output store of the register kernels: SP = 0 streams it (nt), SP = 3
// streams it and writes it through the L2 at device scope (nt sc1; the
// single-stripe store policy, kernels dispatch below).  The trailing s_nop
// keeps the compiler's next instruction from overwriting the data registers
// before the store has read them.
template <int SP>
__device__ __forceinline__ void store16_pol(uint8_t* p, u32x4 v) {
    if constexpr (SP == 3)
        asm volatile("global_store_dwordx4 %0, %1, off nt sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
    else
        store16_out<true>(p, v);
}

// The last (sz % 16) bytes of a block.
__device__ inline u32x4 load_tail(const uint8_t* p, uint32_t nb) {
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    for (uint32_t b = 0; b < nb; ++b) w[b >> 2] |= static_cast<uint32_t>(p[b]) << (8 * (b & 3));
    return u32x4{w[0], w[1], w[2], w[3]};
}

__device__ inline void store_tail(uint8_t* p, u32x4 v, uint32_t nb) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    for (uint32_t b = 0; b < nb; ++b) p[b] = static_cast<uint8_t>(w[b >> 2] >> (8 * (b & 3)));
}

// Walks this lane's (stripe, chunk) units in grid-stride order without a
// division per step.  (An XCD-contiguous workgroup order measured 2 % slower
// on 256 x 1 MiB K=3/M=10 encodes from cold caches, profiles/r02_mb_cold.log.)
struct UnitIter {
    uint32_t s, c;
    template <class J>
    __device__ explicit UnitIter(const J& job) : UnitIter(job, blockIdx.x) {}
    // `block`: the workgroup's index among the job's own workgroups (a paired
    // launch deals its grid across two jobs)
    template <class J>
    __device__ UnitIter(const J& job, uint32_t block) {
        const uint32_t gid = block * kBlock + threadIdx.x;
        s = gid / job.cps;
        c = gid - s * job.cps;
    }
    template <class J>
    __device__ __forceinline__ void next(const J& job) {
        c += job.gs_c;
        s += job.gs_s;
        if (c >= job.cps) {
            c -= job.cps;
            ++s;
        }
    }
};

// Byte span of chunk c of a block of sz bytes.  Chunks are CH bytes; the last
// one, when sz is not a multiple of CH, is shifted back to end at sz and so
// overlaps its neighbour: both lanes compute and store identical bytes there,
// and every lane stays on the full-width load/store path.  Blocks shorter
// than CH, and accumulating launches (XOR into the output is not idempotent),
// take the byte-wise tail instead.
struct Span {
    uint64_t off;
    bool full;
    uint32_t nb;
};

template <uint32_t CH, bool OVERLAP>
__device__ __forceinline__ Span chunk_span(uint32_t c, uint64_t sz, uint32_t nfull) {
    const uint64_t off = static_cast<uint64_t>(c) * CH;
    if (c < nfull) return Span{off, true, CH};
    if (OVERLAP && sz >= CH) return Span{sz - CH, true, CH};
    return Span{off, false, static_cast<uint32_t>(sz - off)};
}

// A kernel's argument block read in place from the kernel-argument segment
// through a pointer the compiler must treat as new at every call (empty asm):
// the loads stay where they are used instead of all being hoisted into the
// prologue, where the table dwords and the block pointers overflow the SGPRs
// and spill to VGPR lanes (v_writelane / v_readlane per wave).
template <class J>
using KPtr = const __attribute__((address_space(4))) J*;

// OFF: the block's byte offset in the argument segment (the second job of a
// paired launch).
template <class J, size_t OFF = 0>
__device__ __forceinline__ KPtr<J> kernarg_job() {
    typedef const __attribute__((address_space(4))) char* KBytes;
    KPtr<J> kj = (KPtr<J>)((KBytes)__builtin_amdgcn_kernarg_segment_ptr() + OFF);
    asm volatile("" : "+s"(kj));
    return kj;
}

// The job where its pointers and tables are read: AL (argument loads) reads
// them in place through kernarg_job, each where it is used; otherwise through
// the argument the compiler loaded in the prologue.
template <bool AL, class J>
__device__ __forceinline__ auto job_at(const J& job) {
    if constexpr (AL)
        return kernarg_job<J>();
    else
        return &job;
}

// ---- the dense batch walk --------------------------------------------------------
// A batch of nstripes stripes of sz bytes each.  A wave's 64 units lie in ONE
// stripe: a stripe gets wps = ceil(cps / 64) waves, the last one partly
// masked, so the stripe number is wave-uniform.  The grid strides over
// (stripe, wave) pairs; fill_walk (below) fills these fields.
struct Walk {
    uint64_t sz;
    uint32_t nstripes, cps;  // cps: 16-byte chunks per stripe
    uint32_t wps;            // waves per stripe
    uint32_t gs_w, gs_s;     // grid stride expressed as (waves, stripes): stride = gs_s*wps + gs_w
    uint32_t pad_;
};

// This wave's index in a grid of workgroups of WG lanes.
template <uint32_t WG = kBlock>
__device__ __forceinline__ uint32_t grid_wave() {
    if constexpr (WG == 64u)
        return blockIdx.x;
    else
        return blockIdx.x * (WG / 64u) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
}

// The (stripe, wave) pairs of one wave, without a division per step:
//   for (WaveWalk it(job.walk, grid_wave()); it.s < n; it.next(job.walk))
// n is the stripe count, or the length of a list whose entries name the
// stripes (pairs_locate, pairs_correct): then s counts entries.
struct WaveWalk {
    uint32_t s, w;
    __device__ __forceinline__ WaveWalk(const Walk& k, uint32_t gw) : s(gw / k.wps), w(gw - s * k.wps) {}
    __device__ __forceinline__ void next(const Walk& k) {
        w += k.gs_w;
        s += k.gs_s;
        if (w >= k.wps) {
            w -= k.wps;
            ++s;
        }
    }
};

// This lane's chunk of wave w of a stripe: chunk w*64 + lane with chunk_span's
// overlapped last chunk; *live: the stripe has that chunk.  OVERLAP = false
// ends the block with the byte tail instead: a kernel that XORs into its
// output (matupdate_reg) must touch every byte exactly once.
template <bool OVERLAP = true>
__device__ __forceinline__ Span wave_unit(const Walk& k, uint32_t w, uint32_t lane, bool* live) {
    const uint32_t c = w * 64u + lane;
    *live = c < k.cps;
    return chunk_span<kChunk, OVERLAP>(c, k.sz, static_cast<uint32_t>(k.sz / kChunk));
}

// ---- one unit: loads, selectors, tables, store (dense and ragged walks alike) ----
// A dead lane loads zeros, a byte tail is zero-filled.
__device__ __forceinline__ u32x4 load_unit(const uint8_t* p, bool live, const Span& sp) {
    if (!live) return u32x4{0u, 0u, 0u, 0u};
    return sp.full ? load16(p) : load_tail(p, sp.nb);
}

// N rows at once, so that all N loads are issued before any of them is used.
template <int N>
__device__ __forceinline__ void load_units(u32x4 (&x)[N], const uint8_t* const (&p)[N], uint64_t off, bool live,
                                           const Span& sp) {
#pragma unroll
    for (int j = 0; j < N; ++j) x[j] = u32x4{0u, 0u, 0u, 0u};
    if (live) {
        if (sp.full) {
#pragma unroll
            for (int j = 0; j < N; ++j) x[j] = load16(p[j] + off);
        } else {
#pragma unroll
            for (int j = 0; j < N; ++j) x[j] = load_tail(p[j] + off, sp.nb);
        }
    }
}

// A streaming store; no byte past the block's end is written.
__device__ __forceinline__ void store_unit(uint8_t* p, u32x4 y, bool live, const Span& sp) {
    if (live) {
        if (sp.full)
            store16_pol<0>(p, y);
        else
            store_tail(p, y, sp.nb);
    }
}

// The selectors of the four dwords of each of K inputs.
template <int K>
__device__ __forceinline__ void unit_sel(Sel (&sel)[4][K], const u32x4 (&x)[K]) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
        sel[0][j] = selectors(x[j].x);
        sel[1][j] = selectors(x[j].y);
        sel[2][j] = selectors(x[j].z);
        sel[3][j] = selectors(x[j].w);
    }
}

// One coefficient's table from its five dwords, in the argument block or in
// device memory read through a constant-address-space pointer (scalar loads).
typedef const __attribute__((address_space(4))) uint32_t* CU32;
__device__ __forceinline__ Tab tab_at(const uint32_t* p) { return Tab{p[0], p[1], p[2], p[3], p[4]}; }
__device__ __forceinline__ Tab tab_at(CU32 p) { return Tab{p[0], p[1], p[2], p[3], p[4]}; }

// The K tables of one matrix row, laid out one after the other from p on.
template <int K, class P>
__device__ __forceinline__ void row_tabs(Tab (&t)[K], P p) {
#pragma unroll
    for (int j = 0; j < K; ++j) t[j] = tab_at(p + j * 5);
}

// ---------------------------------------------------------------------------
// matapply_reg<K, R>: compile-time k and r.  The kernel argument block holds
// the K + R block pointers and the K*R coefficients' tables (5 dwords each):
// 560 bytes for <3,7>, against 2.2 KiB for the table kernels' MatJob.
// ---------------------------------------------------------------------------
template <int K, int R>
struct alignas(16) RegJob {
    uint64_t sz, in_sstride, out_sstride;
    uint32_t nstripes, cps, gs_c, gs_s;
    uint32_t* done_flag;  // pinned host word a one-workgroup launch stores done_seq into when finished
    uint32_t done_seq, pad_;
    const uint8_t* in[K];
    uint8_t* out[R];
    uint32_t tab[K * R * 5];
};

template <int K, int R>
__device__ __forceinline__ Tab reg_table(const RegJob<K, R>& job, uint32_t i) {
    const uint32_t* t = &job.tab[i * 5];
    return Tab{t[0], t[1], t[2], t[3], t[4]};
}

// One (stripe, chunk) unit: load K x 16 bytes, store R x 16 bytes.  AL: each
// row's tables and output pointer are loaded (scalar loads) right before use.
template <int K, int R, int SP, bool AL, size_t OFF = 0>
__device__ __forceinline__ void reg_compute_store(const RegJob<K, R>& job, const Tab (&T)[R][K], const u32x4 (&x)[K],
                                                  uint64_t ob, bool full, uint32_t nb) {
    Sel sel[4][K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        sel[0][j] = selectors(x[j].x);
        sel[1][j] = selectors(x[j].y);
        sel[2][j] = selectors(x[j].z);
        sel[3][j] = selectors(x[j].w);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        Tab t[K];
        uint8_t* out;
        if constexpr (AL) {
            const KPtr<RegJob<K, R>> kj = kernarg_job<RegJob<K, R>, OFF>();
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const uint32_t i = (r * K + j) * 5;
                t[j] = Tab{kj->tab[i], kj->tab[i + 1], kj->tab[i + 2], kj->tab[i + 3], kj->tab[i + 4]};
            }
            out = kj->out[r];
        } else {
#pragma unroll
            for (int j = 0; j < K; ++j) t[j] = T[r][j];
            out = job.out[r];
        }
        const u32x4 y{gf_dot<K>(t, sel[0]), gf_dot<K>(t, sel[1]), gf_dot<K>(t, sel[2]), gf_dot<K>(t, sel[3])};
        if (full)
            store16_pol<SP>(out + ob, y);
        else
            store_tail(out + ob, y, nb);
    }
}

template <int K, int R>
__device__ __forceinline__ void reg_load(const RegJob<K, R>& job, u32x4 (&x)[K], uint64_t ib, bool full,
                                         uint32_t nb) {
    if (full) {
#pragma unroll
        for (int j = 0; j < K; ++j) x[j] = load16(job.in[j] + ib);
    } else {
#pragma unroll
        for (int j = 0; j < K; ++j) x[j] = load_tail(job.in[j] + ib, nb);
    }
}

// PF: the next unit's inputs are loaded before the current unit is computed,
// so a lane with several units (grid-stride) keeps loads in flight while it
// computes (tools/mb_encode.hip, variants "PF"; 5-8 rows only: from cold
// caches the 3-row decode is slower with it, profiles/r02_reg_pf_ab.log).
// SP: output store policy (store16_pol).  AL: tables and output pointers read
// where they are used (reg_compute_store).
template <int K, int R, int SP, bool PF, bool AL, size_t OFF>
__device__ __forceinline__ void reg_body(const RegJob<K, R>& job, uint32_t block) {
    Tab T[R][K];
    if constexpr (!AL) {
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int j = 0; j < K; ++j) T[r][j] = reg_table(job, r * K + j);
    }

    const uint64_t sz = job.sz;
    const uint32_t nfull = static_cast<uint32_t>(sz / kChunk);
    UnitIter u(job, block);
    if constexpr (PF) {
        u32x4 x[K];
        Span sp = chunk_span<kChunk, true>(u.c, sz, nfull);
        uint64_t ob = u.s * job.out_sstride + sp.off;
        if (u.s < job.nstripes) reg_load<K, R>(job, x, u.s * job.in_sstride + sp.off, sp.full, sp.nb);
        while (u.s < job.nstripes) {
            UnitIter v = u;
            v.next(job);
            const Span spn = chunk_span<kChunk, true>(v.c, sz, nfull);
            u32x4 xn[K];
            if (v.s < job.nstripes) reg_load<K, R>(job, xn, v.s * job.in_sstride + spn.off, spn.full, spn.nb);
            reg_compute_store<K, R, SP, AL, OFF>(job, T, x, ob, sp.full, sp.nb);
#pragma unroll
            for (int j = 0; j < K; ++j) x[j] = xn[j];
            sp = spn;
            ob = v.s * job.out_sstride + spn.off;
            u = v;
        }
    } else {
        while (u.s < job.nstripes) {
            const Span sp = chunk_span<kChunk, true>(u.c, sz, nfull);
            u32x4 x[K];
            reg_load<K, R>(job, x, u.s * job.in_sstride + sp.off, sp.full, sp.nb);
            reg_compute_store<K, R, SP, AL, OFF>(job, T, x, u.s * job.out_sstride + sp.off, sp.full, sp.nb);
            u.next(job);
        }
    }
}

// ---- single-stripe, one unit per lane (ONE) -----------------------------------
// A launch of one stripe whose grid covers every 16-byte unit (launch_reg: no
// grid-stride, sz >= 16) needs none of the walk: the lane's unit is its global
// index, there is no stripe to divide out, no next unit to prefetch, and the
// last chunk shifted back to end at sz leaves no byte tail.  reg_body's fixed
// part is the whole life of such a wave (the 64 MiB K=3/M=10 stripe: 5,462
// workgroups of one unit per lane).  Measured on that stripe's encode + decode
// step, interleaved with the walking form: +3.3 % (profiles/r07_reg_one_ab.json).
//
// ZFEC_REG_ONE (A/B knob, tools/ab_build.sh; 0 = every launch walks reg_body)
// ZFEC_REG_TPIPE (with ONE, AL shapes: 1 = the tables of row r+1 are requested
// before row r is computed, row 0's with the header; 0 = each row's tables
// right before use, as reg_compute_store's AL form; the same A/B: medians
// 2557 GB/s without it, 2578 with it, a difference inside the runs' spread)
#ifndef ZFEC_REG_ONE
#define ZFEC_REG_ONE 1
#endif
#ifndef ZFEC_REG_TPIPE
#define ZFEC_REG_TPIPE 1
#endif

// Requests one dword of every 64-byte line of the argument block (scalar
// loads, results unused) so that a launch's first waves, which find the
// scalar cache empty, take those misses at once instead of one per row.  The
// block's base is only known to be 16-byte aligned: offsets 0, 64, ... and the
// last dword reach every line it touches.  The destinations stay allocated
// until the wait, which the header's own wait would make anyway (scalar loads
// return out of order: any wait is for all of them).
template <class J>
struct KernargTouch {
    static constexpr int kLines = (sizeof(J) + 63) / 64;
    uint32_t t[kLines + 1];
    __device__ __forceinline__ void request() {
        typedef const __attribute__((address_space(4))) uint32_t* KWords;
        const KWords base = (KWords)__builtin_amdgcn_kernarg_segment_ptr();
#pragma unroll
        for (int i = 0; i < kLines; ++i)
            asm volatile("s_load_dword %0, %1, %2" : "=s"(t[i]) : "s"(base), "n"(i * 64));
        asm volatile("s_load_dword %0, %1, %2" : "=s"(t[kLines]) : "s"(base), "n"(int(sizeof(J)) - 4));
    }
    __device__ __forceinline__ void wait() {
        __builtin_amdgcn_sched_barrier(0);  // what was requested above stays above
        asm volatile("s_waitcnt lgkmcnt(0)" ::"s"(t[0]));
#pragma unroll
        for (int i = 1; i <= kLines; ++i) asm volatile("" ::"s"(t[i]));
    }
};

template <int K, int R>
struct RowArgs {
    Tab t[K];
    uint8_t* out;
};

// Row r's tables and output pointer, read from the argument segment at this
// point of the program (kernarg_job).
template <int K, int R>
__device__ __forceinline__ RowArgs<K, R> reg_row_args(int r) {
    const KPtr<RegJob<K, R>> kj = kernarg_job<RegJob<K, R>>();
    RowArgs<K, R> a;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const uint32_t i = (r * K + j) * 5;
        a.t[j] = Tab{kj->tab[i], kj->tab[i + 1], kj->tab[i + 2], kj->tab[i + 3], kj->tab[i + 4]};
    }
    a.out = kj->out[r];
    return a;
}

template <int K, int R, int SP, bool AL, bool TP>
__device__ __forceinline__ void reg_body_one(const RegJob<K, R>& job) {
    RowArgs<K, R> cur;
    if constexpr (AL && TP) {
        KernargTouch<RegJob<K, R>> touch;
        touch.request();
        cur = reg_row_args<K, R>(0);
        touch.wait();
    }
    Tab T[R][K];
    if constexpr (!AL) {
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int j = 0; j < K; ++j) T[r][j] = reg_table(job, r * K + j);
    }
    // The lane's chunk; the last one is shifted back to end at sz
    // (chunk_span<kChunk, true>, always full here: sz >= 16), and so is every
    // lane of the last workgroup past it: they store the same bytes again,
    // as overlapping chunks do, and the wave needs no branch.
    const uint64_t sz = job.sz;
    const uint64_t own = static_cast<uint64_t>(blockIdx.x * kBlock + threadIdx.x) * kChunk;
    const uint64_t off = own + kChunk <= sz ? own : sz - kChunk;
    u32x4 x[K];
    reg_load<K, R>(job, x, off, true, kChunk);
    if constexpr (AL && TP) {
        Sel sel[4][K];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            sel[0][j] = selectors(x[j].x);
            sel[1][j] = selectors(x[j].y);
            sel[2][j] = selectors(x[j].z);
            sel[3][j] = selectors(x[j].w);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            RowArgs<K, R> nxt;
            if (r + 1 < R) {
                nxt = reg_row_args<K, R>(r + 1);
                __builtin_amdgcn_sched_barrier(0);  // the requests stay ahead of this row's arithmetic
            }
            const u32x4 y{gf_dot<K>(cur.t, sel[0]), gf_dot<K>(cur.t, sel[1]), gf_dot<K>(cur.t, sel[2]),
                          gf_dot<K>(cur.t, sel[3])};
            store16_pol<SP>(cur.out + off, y);
            if (r + 1 < R) cur = nxt;
        }
    } else {
        reg_compute_store<K, R, SP, AL>(job, T, x, off, true, kChunk);
    }
}

// ONE: 0 = the grid-stride walk (reg_body); 1 = reg_body_one; 2 = reg_body_one
// with pipelined table loads (AL shapes).
template <int K, int R, int SP, bool PF, bool AL, int ONE = 0>
__global__ __launch_bounds__(kBlock) void matapply_reg(const RegJob<K, R> job) {
    if constexpr (ONE != 0) {
        reg_body_one<K, R, SP, AL, ONE == 2>(job);  // never a one-workgroup signalling launch (launch_reg)
        return;
    }
    reg_body<K, R, SP, PF, AL, 0>(job, blockIdx.x);
    // one-workgroup launches of a synchronous small call: publish completion
    // in pinned host memory, so the host need not wait in
    // hipStreamSynchronize (fec_abi.cpp run_single).  Every storing wave waits
    // for its own stores, the workgroup meets at a barrier, and ONE lane
    // releases at system scope and stores the flag (MI355X_MICROARCH.md
    // "Valid forms"): one L2 write-back per call.  (A system fence in every
    // wave before the barrier, round 2's form, cost five write-backs: the
    // kernel took 6.1 us in the trace against 2.6 us for this form,
    // tools/inline_probe.hip, profiles/r03_small_call_kernels.txt.)
    if (job.done_flag) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // system scope
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(job.done_flag, job.done_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// ---------------------------------------------------------------------------
// matapply_one<K>: the synchronous small call from host memory (fec_abi.cpp
// run_single: every block in the thread's pinned bounce buffer, read and
// written over PCIe).  One workgroup, one whole 16-byte unit per lane (the
// bounce buffer's 256-byte slots let a row run to its 16-byte multiple), and
// the output rows in a loop that is not unrolled, each row's tables and
// pointer read from the argument segment where they are used.  A
// one-workgroup launch lands on any XCD and fetches its instructions cold, so
// code size is latency: matapply_reg<3,7> (7.4 KB of code, the unrolled rows
// and the grid-stride walk with its prefetch and tail paths) took 5.5 us in
// the kernel trace against 2.6 us for a stand-in of the same PCIe traffic
// (profiles/r03_small_call_kernels.txt).
// ---------------------------------------------------------------------------
struct alignas(16) OneJob {
    const uint8_t* in[4];
    uint8_t* out[8];
    uint32_t* done_flag;
    uint32_t units, r, done_seq, pad_;
    alignas(16) uint32_t tab[4 * 8 * 5];  // row-major (r, j) coefficient tables, K per row (16-byte loads)
};
static_assert(offsetof(OneJob, tab) % 16 == 0, "matapply_one loads the tables 16 bytes at a time");

// INL: the k input blocks ride in the argument block itself (k x units x 16
// bytes at most kOneInline), which HIP writes to device memory with the
// launch: the kernel reads them there instead of across PCIe from the bounce
// buffer, and the caller's bytes need no copy into pinned memory first
// (tools/inline_probe.hip: 7.2 against 7.9 us launch to completion seen for
// a 4 KiB K=3/M=10 encode stand-in).
constexpr uint32_t kOneInline = kOneInlineBytes;  // a 4 KiB K=3 stripe: 3 x 88 units of 16 bytes = 4,224
struct alignas(16) OneJobInline {
    OneJob job;
    u32x4 data[kOneInline / 16];  // input j's unit u at data[j * units + u]
};

__device__ __forceinline__ const OneJob& one_job(const OneJob& a) { return a; }
__device__ __forceinline__ const OneJob& one_job(const OneJobInline& a) { return a.job; }

template <int K, bool INL, class J>
__global__ __launch_bounds__(kBlock) void matapply_one(const J arg) {
    const OneJob& job = one_job(arg);
    // the coefficient tables (up to 160 dwords) reach LDS in ONE vector load
    // round trip (a lane per 16 bytes of the argument segment), not in a
    // chain of scalar loads per output row
    __shared__ u32x4 stab[4 * 8 * 5 / 4];
    const uint32_t u = threadIdx.x;
    const uint32_t ntab4 = (job.r * K * 5 + 3) / 4;
    if (u < ntab4) {
        const KPtr<OneJob> kj = kernarg_job<OneJob>();
        stab[u] = reinterpret_cast<const __attribute__((address_space(4))) u32x4*>(kj->tab)[u];
    }
    u32x4 x[K];
    if (u < job.units) {
        if constexpr (INL) {
            const KPtr<OneJobInline> kj = kernarg_job<OneJobInline>();
#pragma unroll
            for (int j = 0; j < K; ++j) x[j] = kj->data[j * job.units + u];
        } else {
#pragma unroll
            for (int j = 0; j < K; ++j) x[j] = load16(job.in[j] + size_t(u) * 16);
        }
    }
    __syncthreads();
    if (u < job.units) {
        Sel sel[4][K];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            sel[0][j] = selectors(x[j].x);
            sel[1][j] = selectors(x[j].y);
            sel[2][j] = selectors(x[j].z);
            sel[3][j] = selectors(x[j].w);
        }
        const uint32_t* st = reinterpret_cast<const uint32_t*>(stab);
#pragma unroll 1
        for (uint32_t r = 0; r < job.r; ++r) {
            Tab t[K];
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const uint32_t i = (r * K + j) * 5;
                t[j] = Tab{st[i], st[i + 1], st[i + 2], st[i + 3], st[i + 4]};
            }
            const u32x4 y{gf_dot<K>(t, sel[0]), gf_dot<K>(t, sel[1]), gf_dot<K>(t, sel[2]), gf_dot<K>(t, sel[3])};
            store16_pol<3>(job.out[r] + size_t(u) * 16, y);
        }
    }
    // completion as matapply_reg's: every wave waits for its stores, barrier,
    // one lane's system-scope release, then the flag
    if (job.done_flag) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // system scope
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(job.done_flag, job.done_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

constexpr bool reg_prefetch(int R) { return R >= 5; }
constexpr bool reg_argload(int K, int R) { return K * R * 5 >= 50; }

// ---------------------------------------------------------------------------
// matapply_pair<K, RA, RB>: two independent matrix applications over the same
// k in one launch (fec_run_batch_jobs: e.g. a stripe's encode and another
// stripe's decode), so the pair pays one launch ramp-up and drain instead of
// two.  The grid is both jobs' grids side by side; each workgroup walks its
// own job exactly as matapply_reg would.  RB <= min(RA, K): the second job
// is the narrower one (a decode recovers at most k blocks).
// ---------------------------------------------------------------------------
template <int K, int RA, int RB>
struct alignas(16) PairJob {
    RegJob<K, RA> a;
    RegJob<K, RB> b;
    uint32_t blocks_a, pad_[3];
};

// Job a's workgroups first, then job b's: the dispatcher starts b's as a's
// retire.  (Alternating the two jobs' workgroups measured 10 % slower on the
// cfg2 step, profiles/r03_pair_ab.json.)
template <int K, int RA, int RB, int SP>
__global__ __launch_bounds__(kBlock) void matapply_pair(const PairJob<K, RA, RB> job) {
    using PJ = PairJob<K, RA, RB>;
    constexpr size_t kOffB = offsetof(PJ, b);
    if (blockIdx.x < job.blocks_a)
        reg_body<K, RA, SP, reg_prefetch(RA), reg_argload(K, RA), 0>(job.a, blockIdx.x);
    else
        reg_body<K, RB, SP, reg_prefetch(RB), reg_argload(K, RB), kOffB>(job.b, blockIdx.x - job.blocks_a);
}

// ---------------------------------------------------------------------------
// matapply_rows<K, R>: many stripes of short blocks (1 KiB < sz <= 4 KiB).
// One wave per stripe: lane l owns bytes 16l + 1024h of every block (the last
// chunk shifted back to end at sz), so each wave instruction reads or writes
// one contiguous piece of one block.  The stripe-major unit walk of
// matapply_reg would let a wave instruction straddle the end of one stripe's
// block and the start of the next one's (two DRAM rows); at K=3/M=10 with
// 1366-byte blocks the row walk is 5 % faster (tools/mb_rows.hip).  Every
// piece of the lane's share of the stripe (at most 4) is loaded before any is
// computed, so all of the wave's loads are in flight at once (cfg5 encode
// 67.7 -> 70.1 % of HBM cold, decode 66.7 -> 69.8 %, profiles/r02_rows_pre_ab.log).
// ---------------------------------------------------------------------------
constexpr uint64_t kRowsMin = 1024, kRowsMax = 4096;

template <int K, int R, bool AL>
__global__ __launch_bounds__(kBlock) void matapply_rows(const RegJob<K, R> job) {
    Tab T[R][K];
    if constexpr (!AL) {
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int j = 0; j < K; ++j) T[r][j] = reg_table(job, r * K + j);
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t waves = gridDim.x * (kBlock / 64);
    const uint64_t sz = job.sz;
    for (uint32_t s = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); s < job.nstripes; s += waves) {
        u32x4 x[4][K];
        uint64_t o[4];
        bool live[4];
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const uint64_t off = lane * 16u + 1024u * h;
            live[h] = off < sz;
            o[h] = off + 16u <= sz ? off : sz - 16u;
            if (live[h]) reg_load<K, R>(job, x[h], s * job.in_sstride + o[h], true, 16u);
        }
#pragma unroll
        for (int h = 0; h < 4; ++h)
            if (live[h]) reg_compute_store<K, R, 0, AL>(job, T, x[h], s * job.out_sstride + o[h], true, 16u);
    }
}

// ---------------------------------------------------------------------------
// matapply_mixed<K>: a batched decode whose stripes each have their own
// erasure pattern (fec_decode_batch_mixed), k <= 4, all k primaries out.  The
// K x K tables of every pattern of the call sit in device memory
// (mixed_tab_dwords<K>() dwords per pattern, the Tab layout row-major, padded
// to 16 bytes); ids[s] says which one stripe s uses.
//
// A wave's 64 units lie in ONE stripe: stripe s gets wps = ceil(cps / 64)
// waves, the last one partly masked.  So the stripe, its pattern id and the
// table address are the same in every lane; they are formed through
// readfirstlane and read through constant-address-space pointers, which makes
// the id and the table dwords scalar loads and lets v_perm take the tables as
// SGPR pairs, as in matapply_reg.  (The ids and the tables are written before
// the launch, by a copy or an earlier kernel of the stream, and never by this
// kernel: the scalar cache starts every kernel empty.)  An id >= npatterns
// reads no table and leaves its stripe unwritten.  Blocks under 1 KiB have
// fewer than 64 chunks, so part of each wave idles there.
// ---------------------------------------------------------------------------
template <int K>
constexpr uint32_t mixed_tab_dwords() {
    return (K * K * 5 + 3) / 4 * 4;
}

template <int K>
struct alignas(16) MixedJob {
    Walk walk;
    uint64_t in_sstride, out_sstride;
    uint32_t npatterns;
    const uint32_t* tables;  // npatterns x mixed_tab_dwords<K>()
    const uint32_t* ids;     // nstripes pattern ids
    const uint8_t* in[K];
    uint8_t* out[K];
};

template <int K>
__global__ __launch_bounds__(kBlock) void matapply_mixed(const MixedJob<K> job) {
    constexpr uint32_t TD = mixed_tab_dwords<K>();
    constexpr bool AL = reg_argload(K, K);  // K = 4: each row's tables are read where they are used
    const uint32_t lane = threadIdx.x & 63u;
    const CU32 ids = (CU32)job.ids;
    for (WaveWalk it(job.walk, grid_wave()); it.s < job.walk.nstripes; it.next(job.walk)) {
        const uint32_t s = it.s;
        bool live;
        const Span sp = wave_unit(job.walk, it.w, lane, &live);
        u32x4 x[K];
        load_units<K>(x, job.in, s * job.in_sstride + sp.off, live, sp);
        const uint32_t id = __builtin_amdgcn_readfirstlane(ids[s]);
        if (id < job.npatterns) {
            CU32 tp = (CU32)job.tables + size_t(id) * TD;
            Sel sel[4][K];
            unit_sel<K>(sel, x);
            const uint64_t ob = s * job.out_sstride + sp.off;
#pragma unroll
            for (int r = 0; r < K; ++r) {
                if constexpr (AL) asm volatile("" : "+s"(tp));
                Tab t[K];
                row_tabs<K>(t, tp + r * K * 5);
                const u32x4 y{gf_dot<K>(t, sel[0]), gf_dot<K>(t, sel[1]), gf_dot<K>(t, sel[2]), gf_dot<K>(t, sel[3])};
                store_unit(job.out[r] + ob, y, live, sp);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// matapply_ragged<K, R>: a batch whose stripes each have their own size
// (fec_encode_batch_ragged / fec_decode_batch_ragged), k <= 4, up to 8 rows
// per launch, one matrix for all stripes (its tables in the argument block, as
// RegJob), inside ragged_walk (below).  Per stripe the body tests that it fits
// both arenas (ragged_fits; a stripe that does not is neither read nor
// written) and makes the stripe's wave steps: K rows loaded, R rows stored.
// ---------------------------------------------------------------------------
template <int K, int R>
struct alignas(16) RaggedJob {
    uint64_t in_bstride, out_bstride;  // 0: the stripe's own size (packed objects)
    uint64_t in_bytes, out_bytes;      // extents of the two arenas
    uint32_t nstripes;
    uint32_t rows_all;  // output rows of the whole call (the fit test)
    uint32_t row0;      // this launch stores rows row0 .. row0 + R of them
    uint32_t pad_;
    const uint64_t* ustart;  // nstripes + 1
    const uint64_t* sizes;
    const uint64_t* in_off;
    const uint64_t* out_off;
    const uint8_t* in;
    uint8_t* out;
    uint32_t tab[K * R * 5];
};

typedef const __attribute__((address_space(4))) uint64_t* CU64;

__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v));
    const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v >> 32));
    return (static_cast<uint64_t>(hi) << 32) | lo;
}

// ---------------------------------------------------------------------------
// ragged_walk: the walk every ragged kernel makes.  A unit is one wave step of
// one stripe -- 64 lanes x 16 bytes of every block -- so stripe s has
// ceil(sizes[s] / 1024) units and ustart is their exclusive prefix sum,
// ustart[ns] the total T.
//
// The launch has G waves; wave g owns the contiguous units [g*q + min(g, e),
// ...) with q = T / G, e = T % G (the shard_range rule).  It finds its first
// stripe by one binary search over ustart (the last s with ustart[s] <= first,
// which skips zero-size stripes) and walks forward, calling
// body(stripe, s, u, stop) once per stripe with the wave's units [u, stop) of
// it (none, u == stop, where the range ends on the stripe's first unit).  The
// next stripe's descriptor is requested before the body runs.  Everything
// about a stripe is the same in every lane: it is formed through readfirstlane
// and read through constant-address-space pointers (scalar loads), as in
// matapply_mixed.  The descriptor arrays are written before the launch (a
// copy, ragged_scan or the caller's earlier work in the stream), never by the
// kernel that walks them.  All byte addresses are 64-bit.
//
// RaggedDesc names the arrays: ustart, sizes, NOFF offset arrays and, with
// WORD, one 32-bit word per stripe (a pattern id, a verdict); RaggedStripe is
// one stripe's entry of each.
// ---------------------------------------------------------------------------
template <int NOFF, bool WORD>
struct RaggedDesc {
    uint32_t ns;
    const uint64_t* ustart;  // ns + 1
    const uint64_t* sizes;
    const uint64_t* off[NOFF];
    const uint32_t* word;
};

template <int NOFF, bool WORD>
struct RaggedStripe {
    uint64_t u0, u1;  // its units: [u0, u1)
    uint64_t sz, off[NOFF];
    uint32_t word;
};

template <int NOFF, bool WORD>
__device__ __forceinline__ RaggedStripe<NOFF, WORD> ragged_stripe(const RaggedDesc<NOFF, WORD>& d, uint32_t s) {
    const CU64 us = (CU64)d.ustart;
    RaggedStripe<NOFF, WORD> t;
    t.u0 = us[s];
    t.u1 = us[s + 1];
    t.sz = ((CU64)d.sizes)[s];
#pragma unroll
    for (int i = 0; i < NOFF; ++i) t.off[i] = ((CU64)d.off[i])[s];
    t.word = 0;
    if constexpr (WORD) t.word = ((CU32)d.word)[s];
    return t;
}

template <int NOFF, bool WORD, class Body>
__device__ __forceinline__ void ragged_walk(const RaggedDesc<NOFF, WORD>& d, Body&& body) {
    using Stripe = RaggedStripe<NOFF, WORD>;
    const uint32_t g = blockIdx.x * (kBlock / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t G = gridDim.x * (kBlock / 64);
    const CU64 us = (CU64)d.ustart;
    const uint32_t ns = d.ns;
    const uint64_t total = us[ns];
    // (a launch with a wave per unit or more needs no division)
    const uint64_t q = total <= G ? (total == G ? 1u : 0u) : total / G, e = total - q * G;
    uint64_t u = uniform64(g * q + (g < e ? g : e));
    const uint64_t end = uniform64(g * q + (g < e ? g : e) + q + (g < e ? 1u : 0u));
    if (u >= end) return;
    uint32_t lo = 0, hi = ns;  // ustart[lo] <= u < ustart[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (us[mid] <= u)
            lo = mid;
        else
            hi = mid;
    }
    uint32_t s = __builtin_amdgcn_readfirstlane(lo);
    Stripe cur = ragged_stripe(d, s);
    for (;;) {
        Stripe nxt = cur;
        if (s + 1 < ns) nxt = ragged_stripe(d, s + 1);
        const uint64_t stop = cur.u1 < end ? cur.u1 : end;
        body(cur, s, u, stop);
        u = stop;
        if (u >= end || s + 1 >= ns) break;
        ++s;
        cur = nxt;
        while (cur.u1 == cur.u0 && s + 1 < ns) {  // zero-size stripes
            ++s;
            cur = ragged_stripe(d, s);
        }
    }
}

// chunk_span<kChunk, OVERLAP> with a 64-bit chunk number (a stripe is not
// bounded by 2^32 chunks here: its size is whatever the descriptor says).
template <bool OVERLAP = true>
__device__ __forceinline__ Span ragged_span(uint64_t c, uint64_t sz, uint64_t nfull) {
    const uint64_t off = c * kChunk;
    if (c < nfull) return Span{off, true, kChunk};
    if (OVERLAP && sz >= kChunk) return Span{sz - kChunk, true, kChunk};
    return Span{off, false, static_cast<uint32_t>(sz - off)};
}

// This lane's chunk of unit w of a stripe of sz bytes: chunk w*64 + lane with
// ragged_span's overlapped last chunk; *live: the stripe has that chunk.
// OVERLAP = false ends the block with the byte tail instead, as
// wave_unit<false> does: every byte belongs to exactly one lane of exactly one
// unit, which a kernel that XORs into its output (matupdate_ragged) needs --
// the unit before the tail's may be the last of ANOTHER wave's range.
template <bool OVERLAP = true>
__device__ __forceinline__ Span ragged_unit(uint64_t w, uint32_t lane, uint64_t sz, bool* live) {
    const uint64_t c = w * 64u + lane;
    *live = c < (sz + kChunk - 1) / kChunk;
    return ragged_span<OVERLAP>(c, sz, sz / kChunk);
}

// The lane's address of the next row.  The empty asm keeps it a per-lane
// 64-bit add: left to itself the compiler may form multiples j * B as
// wave-uniform values that live across the unit loop, in SGPRs the walk does
// not have (matlocate_ragged<4,8> spilled two without it).
__device__ __forceinline__ const uint8_t* next_row(const uint8_t* row, uint64_t B) {
    row += B;
    asm volatile("" : "+v"(row));
    return row;
}

template <int K, int R>
__global__ __launch_bounds__(kBlock) void matapply_ragged(const RaggedJob<K, R> job) {
    using J = RaggedJob<K, R>;
    // each row's tables are read where they are used: the walk's own wave-uniform
    // state (two descriptors, the range, the stripe's bases) takes some 50 SGPRs,
    // so the threshold is lower than reg_argload's
    constexpr bool AL = K * R * 5 >= 15;
    Tab T[R][K];
    if constexpr (!AL) {
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const uint32_t* t = &job.tab[(r * K + j) * 5];
                T[r][j] = Tab{t[0], t[1], t[2], t[3], t[4]};
            }
    }
    const uint32_t lane = threadIdx.x & 63u;
    const RaggedDesc<2, false> desc{job.nstripes, job.ustart, job.sizes, {job.in_off, job.out_off}, nullptr};
    ragged_walk(desc, [&](const RaggedStripe<2, false>& cur, uint32_t, uint64_t u, uint64_t stop) {
        const uint64_t sz = cur.sz;
        const uint64_t ib = job.in_bstride ? job.in_bstride : sz, ob = job.out_bstride ? job.out_bstride : sz;
        if (u < stop && ragged_fits(cur.off[0], ib, K, sz, job.in_bytes) &&
            ragged_fits(cur.off[1], ob, job.rows_all, sz, job.out_bytes)) {
            // the arenas' bases are read from the argument segment per stripe: held across the
            // walk in four SGPRs they spill inside the shared walk (<2,1>: 8 where its own had 6)
            const uint8_t* const in0 = kernarg_job<J>()->in + cur.off[0];
            uint8_t* const out0 = kernarg_job<J>()->out + cur.off[1] + job.row0 * ob;
            for (uint64_t w = u - cur.u0, we = stop - cur.u0; w < we; ++w) {
                bool live;
                const Span sp = ragged_unit(w, lane, sz, &live);
                u32x4 x[K];
#pragma unroll
                for (int j = 0; j < K; ++j) x[j] = u32x4{0u, 0u, 0u, 0u};
                if (live) {
                    if (sp.full) {
#pragma unroll
                        for (int j = 0; j < K; ++j) x[j] = load16(in0 + j * ib + sp.off);
                    } else {
#pragma unroll
                        for (int j = 0; j < K; ++j) x[j] = load_tail(in0 + j * ib + sp.off, sp.nb);
                    }
                }
                Sel sel[4][K];
                unit_sel<K>(sel, x);
                // the row address advances per lane: R wave-uniform row bases would
                // live across the unit loop in SGPRs the walk has no room for
                uint8_t* orow = out0 + sp.off;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    Tab t[K];
                    if constexpr (AL) {
                        const KPtr<J> kj = kernarg_job<J>();
#pragma unroll
                        for (int j = 0; j < K; ++j) {
                            const uint32_t i = (r * K + j) * 5;
                            t[j] = Tab{kj->tab[i], kj->tab[i + 1], kj->tab[i + 2], kj->tab[i + 3], kj->tab[i + 4]};
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < K; ++j) t[j] = T[r][j];
                    }
                    const u32x4 y{gf_dot<K>(t, sel[0]), gf_dot<K>(t, sel[1]), gf_dot<K>(t, sel[2]),
                                  gf_dot<K>(t, sel[3])};
                    if (live) {
                        if (sp.full)
                            store16_pol<0>(orow, y);
                        else
                            store_tail(orow, y, sp.nb);
                    }
                    orow += ob;
                }
            }
        }
    });
}

// ---------------------------------------------------------------------------
// ragged_scan: ustart[0 .. n] from sizes[0 .. n) in device memory, for a
// ragged call whose descriptor arrays the host cannot read.  Three launches
// over tiles of kScanTile sizes: each workgroup sums its tile; one workgroup
// turns the tile sums into their exclusive prefix and writes the total to
// ustart[n]; each workgroup scans its tile again from its prefix.  A size
// larger than `maxsz` (the smaller arena: such a stripe fits neither) counts no
// units.  Plain vector stores: matapply_ragged, a later kernel of the stream,
// reads what these wrote through the scalar cache, which starts every kernel
// empty.
// ---------------------------------------------------------------------------
constexpr uint32_t kScanPer = 16, kScanTile = kBlock * kScanPer;

struct ScanJob {
    const uint64_t* sizes;
    uint64_t* ustart;  // n + 1
    uint64_t* tsum;    // one per tile
    uint64_t n, maxsz;
    uint32_t ntiles, pad_;
};

// Exclusive prefix of v over the workgroup's threads; *total: the sum.
__device__ inline uint64_t scan_block(uint64_t v, uint64_t* total) {
    __shared__ uint64_t sh[kBlock];
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < kBlock; d <<= 1) {
        const uint64_t add = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    const uint64_t incl = sh[t];
    *total = sh[kBlock - 1];
    __syncthreads();
    return incl - v;
}

__device__ __forceinline__ uint64_t scan_units(const ScanJob& job, uint64_t i) {
    const uint64_t sz = job.sizes[i];
    return sz > job.maxsz ? 0 : ragged_units_of(sz);
}

// PHASE 0: tile sums; 1: their prefix (one workgroup); 2: ustart
template <int PHASE>
__global__ __launch_bounds__(kBlock) void ragged_scan(const ScanJob job) {
    if constexpr (PHASE == 1) {
        uint64_t carry = 0;
        for (uint32_t base = 0; base < job.ntiles; base += kBlock) {
            const uint32_t i = base + threadIdx.x;
            const uint64_t v = i < job.ntiles ? job.tsum[i] : 0;
            uint64_t total;
            const uint64_t ex = scan_block(v, &total);
            if (i < job.ntiles) job.tsum[i] = carry + ex;
            carry += total;
        }
        if (threadIdx.x == 0) job.ustart[job.n] = carry;
    } else {
        const uint64_t i0 = (uint64_t(blockIdx.x) * kBlock + threadIdx.x) * kScanPer;
        uint64_t v[kScanPer], sum = 0;
#pragma unroll
        for (uint32_t i = 0; i < kScanPer; ++i) {
            v[i] = i0 + i < job.n ? scan_units(job, i0 + i) : 0;
            sum += v[i];
        }
        uint64_t total;
        uint64_t at = scan_block(sum, &total);
        if constexpr (PHASE == 0) {
            if (threadIdx.x == 0) job.tsum[blockIdx.x] = total;
        } else {
            at += job.tsum[blockIdx.x];
#pragma unroll
            for (uint32_t i = 0; i < kScanPer; ++i) {
                if (i0 + i < job.n) job.ustart[i0 + i] = at;
                at += v[i];
            }
        }
    }
}

// ---------------------------------------------------------------------------
// matverify_reg<K, R>: parity verification (fec_verify_batch), k <= 4 and up
// to 8 check rows per launch.  The R rows matapply_reg<K, R> would store are
// computed in registers from the K basis blocks and compared with the R
// stored check blocks: the launch reads K + R rows and writes nothing unless a
// row differs.  WaveWalk: the stripe number is wave-uniform.  Per unit all
// K + R loads are issued before any arithmetic; per row computed ^ stored, the
// row's syndrome (four words), replaces the stored row in its registers, its
// words are OR-ed, one ballot turns "any lane differs" into one bit of a
// wave-uniform mask, and if the mask is nonzero ONE lane issues one relaxed
// device-scope fetch_or per touched word of the stripe's mismatch words.  Dead
// lanes (past the stripe's last chunk) hold zeros on both sides; the byte tail
// is zero-filled on both sides by load_tail; the overlapped last chunk of
// chunk_span compares some bytes twice, which is harmless.  OR is
// order-independent, so the result is deterministic.
//
// matlocate_reg<K, R>: single-block error location (fec_locate_batch), k <= 4
// and 2 <= R <= 8 checks, all in one launch (bit0 = 0).  The same body
// (scrub_body, LOC choosing the family) down to the mask.  Only under a scalar
// branch on mask != 0 the K hypotheses "only basis slot j is corrupt" are
// tested: the syndromes of such an error satisfy s_r = Q[r][j] . s_0 (Q[r][j] =
// P[r][j] / P[0][j]) at every byte, so a lane where some s_r ^ Q[r][j] . s_0 is
// nonzero refutes j, and one ballot per j gives the wave's excluded bits.  A
// wave whose syndromes are all zero refutes nothing, so skipping it loses
// nothing.  The Q tables sit behind the verify tables in the argument block
// and are read through the kernel-argument pointer inside the branch only: the
// clean path carries no SGPRs for them, performs no store and no atomic.  One
// lane then ORs mismatch bits (from bit 0) and excluded bits (from bit xbit)
// into the stripe's working words.
// ---------------------------------------------------------------------------
template <int K, int R, bool LOC>
struct alignas(16) ScrubJob {
    Walk walk;
    uint64_t sstride;
    uint32_t words;  // mismatch (verify) or working (locate) words per stripe
    uint32_t bit0;   // bit index of this launch's first check row
    uint32_t xbit;   // bit index of basis slot 0's excluded bit (locate)
    uint32_t* bits;
    const uint8_t* in[K];
    const uint8_t* chk[R];
    uint32_t tab[K * R * 5];                   // the RegJob layout: row i, input j at (i*K + j)*5
    uint32_t qtab[LOC ? K * (R - 1) * 5 : 1];  // Q[r][j], r = 1..R-1, at ((r-1)*K + j)*5
};

// ORs `bits` (bit 0 = bit index `bit` of the stripe's words) into the words at
// `base`: one atomic per touched word, issued by the calling lane.
__device__ __forceinline__ void mismatch_or(uint32_t* base, uint32_t bit, uint32_t bits) {
    const uint64_t m = static_cast<uint64_t>(bits) << (bit & 31u);
    uint32_t* wp = base + (bit >> 5);
    const uint32_t lo = static_cast<uint32_t>(m), hi = static_cast<uint32_t>(m >> 32);
    if (lo) (void)__hip_atomic_fetch_or(wp, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (hi) (void)__hip_atomic_fetch_or(wp + 1, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// <1,8> and <3,3> sit at the SGPR limit as matverify_reg shapes (106 and 105)
// and would spill with the dirty branch's registers on top: they too read
// tables and pointers where they are used.  So does <1,7> (100 SGPRs): with
// its tables held it takes 72 VGPRs through scrub_body, a wave per SIMD fewer.
constexpr bool locate_argload(int K, int R) {
    return reg_argload(K, R) || K * R * 5 + 2 * (K + R) >= 56 || (K == 1 && R == 7);
}

template <int K, int R, bool LOC>
__device__ __forceinline__ void scrub_body(const ScrubJob<K, R, LOC>& job) {
    using J = ScrubJob<K, R, LOC>;
    // each row's tables are read where they are used; the block pointers too,
    // so they do not sit in SGPRs next to the tables (<4,8> spilled otherwise)
    constexpr bool AL = LOC ? locate_argload(K, R) : reg_argload(K, R);
    const uint32_t lane = threadIdx.x & 63u;
    for (WaveWalk it(job.walk, grid_wave()); it.s < job.walk.nstripes; it.next(job.walk)) {
        bool live;
        const Span sp = wave_unit(job.walk, it.w, lane, &live);
        // K + R loads under ONE test of live and sp.full, written out: through
        // load_units (one call per array, or one over K + R pointers) a third of
        // the forms take more VGPRs and some lose a wave per SIMD
        u32x4 x[K], y[R];
#pragma unroll
        for (int j = 0; j < K; ++j) x[j] = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int r = 0; r < R; ++r) y[r] = u32x4{0u, 0u, 0u, 0u};
        if (live) {
            const uint64_t ib = it.s * job.sstride + sp.off;
            const auto kj = job_at<AL>(job);
            const uint8_t* in[K];
            const uint8_t* chk[R];
#pragma unroll
            for (int j = 0; j < K; ++j) in[j] = kj->in[j];
#pragma unroll
            for (int r = 0; r < R; ++r) chk[r] = kj->chk[r];
            if (sp.full) {
#pragma unroll
                for (int j = 0; j < K; ++j) x[j] = load16(in[j] + ib);
#pragma unroll
                for (int r = 0; r < R; ++r) y[r] = load16(chk[r] + ib);
            } else {
#pragma unroll
                for (int j = 0; j < K; ++j) x[j] = load_tail(in[j] + ib, sp.nb);
#pragma unroll
                for (int r = 0; r < R; ++r) y[r] = load_tail(chk[r] + ib, sp.nb);
            }
        }
        Sel sel[4][K];
        unit_sel<K>(sel, x);
        uint32_t mask = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            Tab t[K];
            auto kj = job_at<AL>(job);
            // as scrub_ragged_body: the pointer is formed after the previous row's
            // ballot, so at most two rows' tables are in SGPRs at a time
            // (matlocate_reg<4,6> and <4,7> spilled 7 and 36 SGPRs without it)
            if constexpr (AL && LOC) asm volatile("" : "+s"(kj) : "s"(mask));
            row_tabs<K>(t, kj->tab + r * K * 5);
            // the syndrome of row r replaces the stored row
            y[r].x ^= gf_dot<K>(t, sel[0]);
            y[r].y ^= gf_dot<K>(t, sel[1]);
            y[r].z ^= gf_dot<K>(t, sel[2]);
            y[r].w ^= gf_dot<K>(t, sel[3]);
            const uint32_t d = y[r].x | y[r].y | y[r].z | y[r].w;
            if (__builtin_amdgcn_ballot_w64(d != 0u) != 0ull) mask |= 1u << r;
        }
        if (mask != 0u) {  // wave-uniform: a scalar branch, not taken on clean data
            uint32_t excl = 0;
            if constexpr (LOC) {
                const Sel z[4][1] = {{selectors(y[0].x)}, {selectors(y[0].y)}, {selectors(y[0].z)}, {selectors(y[0].w)}};
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    uint32_t d = 0;
#pragma unroll
                    for (int r = 1; r < R; ++r) {
                        const Tab q[1] = {tab_at(kernarg_job<J>()->qtab + ((r - 1) * K + j) * 5)};
                        d |= (y[r].x ^ gf_dot<1>(q, z[0])) | (y[r].y ^ gf_dot<1>(q, z[1])) |
                             (y[r].z ^ gf_dot<1>(q, z[2])) | (y[r].w ^ gf_dot<1>(q, z[3]));
                    }
                    if (__builtin_amdgcn_ballot_w64(d != 0u) != 0ull) excl |= 1u << j;
                }
            }
            if (lane == 0u) {
                uint32_t* const base = job.bits + size_t(it.s) * job.words;
                mismatch_or(base, LOC ? 0u : job.bit0, mask);
                if (LOC && excl != 0u) mismatch_or(base, job.xbit, excl);
            }
        }
    }
}

template <int K, int R>
__global__ __launch_bounds__(kBlock) void matverify_reg(const ScrubJob<K, R, false> job) {
    scrub_body<K, R, false>(job);
}

template <int K, int R>
__global__ __launch_bounds__(kBlock) void matlocate_reg(const ScrubJob<K, R, true> job) {
    scrub_body<K, R, true>(job);
}

// ---------------------------------------------------------------------------
// matrepair_mixed<K, R>: a batched repair whose stripes each have their own
// pattern (fec_repair_batch), k <= 4 and up to 8 output rows per launch.  It is
// matapply_mixed<K> with R rows instead of K: WaveWalk (a wave's 64 units lie
// in ONE stripe), the stripe's id and its record address wave-uniform,
// formed through readfirstlane and read through constant-address-space
// pointers, so ids, mask and tables are scalar loads and v_perm takes the
// tables as SGPR pairs.
//
// A pattern's record in device memory holds the tables of ALL its target rows
// (a call with more than 8 targets is several launches over one upload), the
// Tab layout row-major, then one dword live-row mask: bit i is set when target
// i is a block to rebuild.  Records are padded to 16 bytes.  A launch takes
// rows [bit0, bit0 + R): tab_off is its first row's dword offset in a record.
// A row whose mask bit is clear is skipped by a scalar branch: no table load,
// no arithmetic and no store, so none of its bytes is touched.  An id >=
// npatterns reads no record and leaves its stripe unwritten.  Each row's
// tables (and, for the larger shapes, its output pointer) are read where they
// are used (the pin on the record pointer, job_at for the pointer).
// ---------------------------------------------------------------------------
template <int K, int R>
struct alignas(16) RepairJob {
    Walk walk;
    uint64_t in_sstride, out_sstride;
    uint32_t npatterns;
    uint32_t rec_dwords;     // dwords per pattern record
    uint32_t tab_off;        // dword offset in a record of this launch's first row
    uint32_t mask_off;       // dword offset in a record of the live-row mask
    uint32_t bit0;           // mask bit of this launch's first row
    const uint32_t* records;  // npatterns x rec_dwords
    const uint32_t* ids;      // nstripes pattern ids
    const uint8_t* in[K];
    uint8_t* out[R];
};

template <int K, int R>
__global__ __launch_bounds__(kBlock) void matrepair_mixed(const RepairJob<K, R> job) {
    constexpr bool AL = reg_argload(K, R);  // each row's tables are read where they are used
    const uint32_t lane = threadIdx.x & 63u;
    const CU32 ids = (CU32)job.ids;
    for (WaveWalk it(job.walk, grid_wave()); it.s < job.walk.nstripes; it.next(job.walk)) {
        const uint32_t s = it.s;
        bool live;
        const Span sp = wave_unit(job.walk, it.w, lane, &live);
        u32x4 x[K];
        load_units<K>(x, job.in, s * job.in_sstride + sp.off, live, sp);
        const uint32_t id = __builtin_amdgcn_readfirstlane(ids[s]);
        if (id < job.npatterns) {
            const CU32 rp = (CU32)job.records + size_t(id) * job.rec_dwords;
            const uint32_t mask = __builtin_amdgcn_readfirstlane(rp[job.mask_off]) >> job.bit0;
            CU32 tp = rp + job.tab_off;
            Sel sel[4][K];
            unit_sel<K>(sel, x);
            const uint64_t ob = s * job.out_sstride + sp.off;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if ((mask >> r) & 1u) {  // wave-uniform: a scalar branch
                    if constexpr (AL) asm volatile("" : "+s"(tp));
                    Tab t[K];
                    row_tabs<K>(t, tp + r * K * 5);
                    const u32x4 y{gf_dot<K>(t, sel[0]), gf_dot<K>(t, sel[1]), gf_dot<K>(t, sel[2]),
                                  gf_dot<K>(t, sel[3])};
                    store_unit(job_at<AL>(job)->out[r] + ob, y, live, sp);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------
// matupdate_reg<C, R>: the parity update of changed primaries
// (fec_update_batch): every stripe carries up to C input slots, each the delta
// (or the old and the new bytes) of one primary whose number is the stripe's
// own, and R stored rows are brought up to date in place:
//   row_i ^= sum over the live slots c of E[block_nums[i]][j_c] * d_c.
// Only one column of E per slot is involved, so the kernel does not depend on
// the code's k.  It has matrepair_mixed's shape with one "pattern" per
// primary: record j in device memory holds the tables of E[block_nums[i]][j]
// for ALL the call's rows (a call with more than 8 rows is several launches
// over one upload), one Tab per row, then the live-row mask, one dword per 32
// rows: bit i is set when the coefficient is not zero.  Records are padded to
// 16 bytes.  A launch takes rows [g0, g0 + R), g0 a multiple of 8: tab_off is
// its first row's dword offset in a record, mask_off the dword with its mask
// bits and bit0 its first bit there.
//
// The stripe's C numbers are read through a constant-address-space pointer and
// readfirstlane: scalar loads, wave-uniform, and every branch on them is a
// scalar branch.  A slot whose number is not < k (FEC_UPDATE_NONE, or a
// device-side number out of range) loads nothing and contributes x = 0, so
// its table pointer only has to be valid (record 0).  The row mask is the OR
// of the live slots' masks; a row whose bit is clear is neither read nor
// written, and a stripe with no live slot is left alone.  The loads of the
// live rows are issued before the first of them is used; each row's tables
// are read where they are used (the pin on the record pointers, job_at for
// the row pointer), as in matrepair_mixed.
//
// This is the one register kernel that XORs into its output, so a block ends
// with the byte tail (wave_unit<false>), never with the overlapped last chunk:
// two lanes storing the same bytes would apply the delta twice, or race.
// ---------------------------------------------------------------------------
template <int C, int R>
struct alignas(16) UpdateJob {
    Walk walk;
    uint64_t in_sstride, row_sstride;
    uint32_t k;           // records (one per primary)
    uint32_t rec_dwords;  // dwords per record
    uint32_t tab_off;     // dword offset in a record of this launch's first row
    uint32_t mask_off;    // dword offset in a record of the mask dword of this launch's rows
    uint32_t bit0;        // bit in that dword of this launch's first row
    uint32_t has_old;     // 0: nw holds the deltas
    const uint32_t* records;  // k x rec_dwords
    const uint32_t* changed;  // nstripes x C primary numbers
    const uint8_t* nw[C];
    const uint8_t* od[C];
    uint8_t* row[R];
};

template <int C, int R>
__global__ __launch_bounds__(kBlock) void matupdate_reg(const UpdateJob<C, R> job) {
    constexpr bool AL = reg_argload(C, R);  // each row's tables are read where they are used
    const uint32_t lane = threadIdx.x & 63u;
    const CU32 ch = (CU32)job.changed;
    for (WaveWalk it(job.walk, grid_wave()); it.s < job.walk.nstripes; it.next(job.walk)) {
        const uint32_t s = it.s;
        bool live;
        const Span sp = wave_unit<false>(job.walk, it.w, lane, &live);
        const uint64_t ib = s * job.in_sstride + sp.off;
        u32x4 xn[C], xo[C];
        CU32 tp[C];
        uint32_t mask = 0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            xn[c] = xo[c] = u32x4{0u, 0u, 0u, 0u};
            tp[c] = (CU32)job.records + job.tab_off;
            const uint32_t j = __builtin_amdgcn_readfirstlane(ch[size_t(s) * C + c]);
            if (j < job.k) {  // wave-uniform: a scalar branch
                const CU32 rp = (CU32)job.records + size_t(j) * job.rec_dwords;
                mask |= __builtin_amdgcn_readfirstlane(rp[job.mask_off]);
                tp[c] = rp + job.tab_off;
                xn[c] = load_unit(job.nw[c] + ib, live, sp);
                if (job.has_old) xo[c] = load_unit(job.od[c] + ib, live, sp);
            }
        }
        mask = (mask >> job.bit0) & ((1u << R) - 1u);
        if (mask) {
            const uint64_t ob = s * job.row_sstride + sp.off;
            u32x4 y[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                y[r] = u32x4{0u, 0u, 0u, 0u};
                if ((mask >> r) & 1u) y[r] = load_unit(job_at<AL>(job)->row[r] + ob, live, sp);
            }
            u32x4 x[C];
#pragma unroll
            for (int c = 0; c < C; ++c) x[c] = xn[c] ^ xo[c];
            Sel sel[4][C];
            unit_sel<C>(sel, x);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if ((mask >> r) & 1u) {
                    Tab t[C];
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        if constexpr (AL) asm volatile("" : "+s"(tp[c]));
                        t[c] = tab_at(tp[c] + r * 5);
                    }
                    const u32x4 v{y[r].x ^ gf_dot<C>(t, sel[0]), y[r].y ^ gf_dot<C>(t, sel[1]),
                                  y[r].z ^ gf_dot<C>(t, sel[2]), y[r].w ^ gf_dot<C>(t, sel[3])};
                    store_unit(job_at<AL>(job)->row[r] + ob, v, live, sp);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------
// matupdate_ragged<C, R>: the parity update of a batch whose stripes each have
// their own size (fec_update_batch_ragged), any k: matupdate_reg's wave step
// inside ragged_walk.  The records are matupdate_reg's, unchanged (one per
// primary: a Tab per row of the call, then the live-row mask dwords); the
// arenas, descriptors and fit test are matrepair_ragged's, the input side over
// C slots and the row side over ALL the call's rows.  A launch takes rows
// [row0, row0 + R) of every stripe, row0 a multiple of 8.
//
// Per stripe: the C numbers at changed[s * C + c] come by scalar loads and
// readfirstlane; a slot whose number is not < k is not read (its bit in
// `slots` stays clear, its table pointer is record 0's: valid, multiplied by
// x = 0).  The row mask is the OR of the live slots' masks; a row whose bit is
// clear is neither read nor written, and a stripe with no live row in this
// launch, one that does not fit either side, or an empty one costs scalar work
// only.  Numbers, masks and table pointers are formed inside the stripe's own
// scope: nothing carries from one stripe of a wave's range to the next.
//
// Per unit every load -- the live slots' inputs, then the live rows -- is
// issued before the first store, and each row's tables are read where they are
// used (the pins on the row's dword offset and on the masks).  Row and slot
// addresses advance per lane (next_row).
//
// The block end is the byte tail (ragged_unit<false>): the kernel XORs into
// its output, and in this walk the unit that holds the tail of a stripe of
// 1024 w + t bytes, 0 < t < 16, may be the first of one wave's range while the
// unit before it is the last of another's.  An overlapped last chunk would
// read 16 - t bytes that wave has, or has not yet, updated, and apply the
// delta to them again.  Records, numbers and descriptors are written before
// the launch, never by this kernel, so the scalar reads are coherent.
// ---------------------------------------------------------------------------
struct alignas(16) RaggedUpdateJob {
    uint64_t in_bstride, row_bstride;  // 0: the stripe's own size (packed objects)
    uint64_t in_bytes, row_bytes;      // extents of the input arenas (each) and of the row arena
    uint32_t nstripes;
    uint32_t rows_all;    // stored rows per stripe of the whole call (the fit test)
    uint32_t row0;        // this launch takes rows row0 .. row0 + R
    uint32_t k;           // records (one per primary)
    uint32_t rec_dwords;  // dwords per record
    uint32_t tab_off;     // dword offset in a record of this launch's first row
    uint32_t mask_off;    // dword offset in a record of the mask dword of this launch's rows
    uint32_t bit0;        // bit in that dword of this launch's first row
    const uint64_t* ustart;  // nstripes + 1
    const uint64_t* sizes;
    const uint64_t* in_off;
    const uint64_t* row_off;
    const uint32_t* records;  // k x rec_dwords
    const uint32_t* changed;  // nstripes x C primary numbers
    const uint8_t* nw;
    const uint8_t* od;  // null: nw holds the deltas
    uint8_t* rows;
};

template <int C, int R>
__global__ __launch_bounds__(kBlock) void matupdate_ragged(const RaggedUpdateJob job) {
    using J = RaggedUpdateJob;
    const uint32_t lane = threadIdx.x & 63u;
    const RaggedDesc<2, false> desc{job.nstripes, job.ustart, job.sizes, {job.in_off, job.row_off}, nullptr};
    ragged_walk(desc, [&](const RaggedStripe<2, false>& cur, uint32_t s, uint64_t u, uint64_t stop) {
        const uint64_t sz = cur.sz;
        const uint64_t ib = job.in_bstride ? job.in_bstride : sz, ob = job.row_bstride ? job.row_bstride : sz;
        // the launch's record geometry is read from the argument segment where a stripe needs
        // it, not kept in SGPRs across the walk
        const KPtr<J> kj = kernarg_job<J>();
        if (u < stop && ragged_fits(cur.off[0], ib, C, sz, job.in_bytes) &&
            ragged_fits(cur.off[1], ob, job.rows_all, sz, job.row_bytes)) {
            // this stripe's numbers, table pointers and masks: formed here, dead at the closing brace
            const CU32 ch = (CU32)kj->changed + size_t(s) * C;
            const uint32_t nrec = kj->k;
            CU32 tp[C];
            uint32_t slots = 0, smask = 0;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                tp[c] = (CU32)kj->records + kj->tab_off;
                const uint32_t j = __builtin_amdgcn_readfirstlane(ch[c]);
                if (j < nrec) {  // wave-uniform: a scalar branch
                    const CU32 rp = (CU32)kj->records + size_t(j) * kj->rec_dwords;
                    smask |= __builtin_amdgcn_readfirstlane(rp[kj->mask_off]);
                    tp[c] = rp + kj->tab_off;
                    slots |= 1u << c;
                }
                // said to be wave-uniform once more: left to itself the compiler may choose between
                // the two pointers per lane, and the pin below wants an SGPR pair
                tp[c] = (CU32)uniform64((uint64_t)tp[c]);
            }
            smask = (smask >> kj->bit0) & ((1u << R) - 1u);
            if (smask != 0u) {  // wave-uniform: a stripe with no live row here is not read
                // the arenas' bases, as matrepair_ragged's
                const uint8_t* const nw0 = kj->nw + cur.off[0];
                const uint8_t* const od0 = kj->od ? kj->od + cur.off[0] : nullptr;
                uint8_t* const row0 = kj->rows + cur.off[1] + kj->row0 * ob;
                for (uint64_t w = u - cur.u0, we = stop - cur.u0; w < we; ++w) {
                    // opaque per unit: the row and slot tests stay bit tests of one SGPR each
                    uint32_t mask = smask, sl = slots;
                    asm volatile("" : "+s"(mask), "+s"(sl));
                    bool live;
                    const Span sp = ragged_unit<false>(w, lane, sz, &live);
                    // one pair of lane branches (live, full) around all the loads; inside them the
                    // slot and row tests are scalar branches.  A dead lane and a none slot hold zeros.
                    u32x4 x[C], xo[C], y[R];
#pragma unroll
                    for (int c = 0; c < C; ++c) x[c] = xo[c] = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
                    for (int r = 0; r < R; ++r) y[r] = u32x4{0u, 0u, 0u, 0u};
                    const auto load_all = [&](auto ld) {
                        const uint8_t* in = nw0 + sp.off;
#pragma unroll
                        for (int c = 0; c < C; ++c, in = next_row(in, ib))
                            if ((sl >> c) & 1u) x[c] = ld(in);
                        if (od0) {  // wave-uniform
                            in = od0 + sp.off;
#pragma unroll
                            for (int c = 0; c < C; ++c, in = next_row(in, ib))
                                if ((sl >> c) & 1u) xo[c] = ld(in);
                        }
                        const uint8_t* row = row0 + sp.off;
#pragma unroll
                        for (int r = 0; r < R; ++r, row = next_row(row, ob))
                            if ((mask >> r) & 1u) y[r] = ld(row);
                    };
                    if (live) {
                        if (sp.full)
                            load_all([](const uint8_t* p) { return load16(p); });
                        else
                            load_all([&](const uint8_t* p) { return load_tail(p, sp.nb); });
                    }
#pragma unroll
                    for (int c = 0; c < C; ++c) x[c] = x[c] ^ xo[c];
                    Sel sel[4][C];
                    unit_sel<C>(sel, x);
                    uint8_t* orow = row0 + sp.off;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        if ((mask >> r) & 1u) {  // wave-uniform: a scalar branch
                            Tab t[C];
#pragma unroll
                            for (int c = 0; c < C; ++c) {
                                // the row's offset is opaque here, so its tables are read here
                                uint32_t at = r * 5;
                                asm volatile("" : "+s"(at));
                                t[c] = tab_at(tp[c] + at);
                            }
                            const u32x4 v{y[r].x ^ gf_dot<C>(t, sel[0]), y[r].y ^ gf_dot<C>(t, sel[1]),
                                          y[r].z ^ gf_dot<C>(t, sel[2]), y[r].w ^ gf_dot<C>(t, sel[3])};
                            store_unit(orow, v, live, sp);
                        }
                        orow += ob;
                    }
                }
            }
        }
    });
}

// ---------------------------------------------------------------------------
// rows_differ: the second step of parity verification for the shapes
// matverify_reg does not take.  The expected check rows were computed into
// scratch (a) by whatever kernel apply_matrix picks; this kernel compares them
// with the stored rows (b): run-time r <= kMaxOut, WaveWalk and scrub_body's
// ballot-then-OR reduction.  Rows go in groups of 4 so that 8 loads are in
// flight before the first comparison.
// ---------------------------------------------------------------------------
struct alignas(16) DifferJob {
    Walk walk;
    uint64_t a_sstride, b_sstride;
    uint32_t words, bit0, r;
    uint32_t* mismatch;
    const uint8_t* a[kMaxOut];
    const uint8_t* b[kMaxOut];
};

__global__ __launch_bounds__(kBlock) void rows_differ(const DifferJob job) {
    constexpr uint32_t G = 4;
    const uint32_t lane = threadIdx.x & 63u;
    for (WaveWalk it(job.walk, grid_wave()); it.s < job.walk.nstripes; it.next(job.walk)) {
        bool live;
        const Span sp = wave_unit(job.walk, it.w, lane, &live);
        const uint64_t ao = it.s * job.a_sstride + sp.off, bo = it.s * job.b_sstride + sp.off;
        uint32_t* const base = job.mismatch + size_t(it.s) * job.words;
        for (uint32_t r0 = 0; r0 < job.r; r0 += G) {
            const uint32_t n = job.r - r0 < G ? job.r - r0 : G;
            u32x4 p[G], q[G];
#pragma unroll
            for (uint32_t i = 0; i < G; ++i) {
                p[i] = q[i] = u32x4{0u, 0u, 0u, 0u};
                if (i < n) {
                    p[i] = load_unit(job.a[r0 + i] + ao, live, sp);
                    q[i] = load_unit(job.b[r0 + i] + bo, live, sp);
                }
            }
            uint32_t mask = 0;
#pragma unroll
            for (uint32_t i = 0; i < G; ++i) {
                const u32x4 d = p[i] ^ q[i];
                if (__builtin_amdgcn_ballot_w64((d.x | d.y | d.z | d.w) != 0u) != 0ull) mask |= 1u << i;
            }
            if (mask != 0u && lane == 0u) mismatch_or(base, job.bit0 + r0, mask);
        }
    }
}

// ---------------------------------------------------------------------------
// rows_locate: rows_differ's place in fec_locate_batch for the shapes
// matlocate_reg does not take.  a holds the expected check rows (scratch), b
// the stored ones; a launch takes rows [bit0, bit0 + r) of the c checks, r <=
// kMaxOut, and always reads row 0's pair too, so every launch has s_0.  The
// group's mismatch bits are OR-ed out as rows_differ does.  Only a wave that
// saw a nonzero syndrome (s_0 or one of its rows) tests the k hypotheses
// against its rows: the syndromes are re-read (from L2), Q[i][j]'s table comes
// from device memory by wave-uniform scalar loads ((i-1)*k + j)*5 dwords into
// qtab, written by a copy before the launch), and the excluded bits go out 32
// basis slots at a time.  Dirty units are rare; their speed is not a goal.
// ---------------------------------------------------------------------------
struct alignas(16) LocateRowsJob {
    Walk walk;
    uint64_t a_sstride, b_sstride;
    uint32_t words, bit0, r;
    uint32_t k, xbit, pad_;
    uint32_t* bits;
    const uint32_t* qtab;
    const uint8_t* a0;  // row 0's pair
    const uint8_t* b0;
    const uint8_t* a[kMaxOut];
    const uint8_t* b[kMaxOut];
};

__global__ __launch_bounds__(kBlock) void rows_locate(const LocateRowsJob job) {
    constexpr uint32_t G = 4;
    const uint32_t lane = threadIdx.x & 63u;
    const CU32 qtab = (CU32)job.qtab;
    for (WaveWalk it(job.walk, grid_wave()); it.s < job.walk.nstripes; it.next(job.walk)) {
        bool live;
        const Span sp = wave_unit(job.walk, it.w, lane, &live);
        const uint64_t ao = it.s * job.a_sstride + sp.off, bo = it.s * job.b_sstride + sp.off;
        uint32_t* const base = job.bits + size_t(it.s) * job.words;
        // s_0: the first group has it as its row 0, a later group reads the pair again
        u32x4 s0{0u, 0u, 0u, 0u};
        bool dirty = false;
        if (job.bit0 != 0u) {
            s0 = load_unit(job.a0 + ao, live, sp) ^ load_unit(job.b0 + bo, live, sp);
            dirty = __builtin_amdgcn_ballot_w64((s0.x | s0.y | s0.z | s0.w) != 0u) != 0ull;
        }
        for (uint32_t r0 = 0; r0 < job.r; r0 += G) {
            const uint32_t n = job.r - r0 < G ? job.r - r0 : G;
            u32x4 p[G], q[G];
#pragma unroll
            for (uint32_t i = 0; i < G; ++i) {
                p[i] = q[i] = u32x4{0u, 0u, 0u, 0u};
                if (i < n) {
                    p[i] = load_unit(job.a[r0 + i] + ao, live, sp);
                    q[i] = load_unit(job.b[r0 + i] + bo, live, sp);
                }
            }
            if (r0 == 0u && job.bit0 == 0u) s0 = p[0] ^ q[0];
            uint32_t mask = 0;
#pragma unroll
            for (uint32_t i = 0; i < G; ++i) {
                const u32x4 d = p[i] ^ q[i];
                if (__builtin_amdgcn_ballot_w64((d.x | d.y | d.z | d.w) != 0u) != 0ull) mask |= 1u << i;
            }
            if (mask != 0u) {
                dirty = true;
                if (lane == 0u) mismatch_or(base, job.bit0 + r0, mask);
            }
        }
        if (dirty) {  // wave-uniform
            const Sel z[4][1] = {{selectors(s0.x)}, {selectors(s0.y)}, {selectors(s0.z)}, {selectors(s0.w)}};
            for (uint32_t j0 = 0; j0 < job.k; j0 += 32u) {
                const uint32_t nj = job.k - j0 < 32u ? job.k - j0 : 32u;
                uint32_t excl = 0;
                for (uint32_t i = 0; i < job.r; ++i) {
                    const uint32_t gi = job.bit0 + i;
                    if (gi == 0u) continue;  // s_0 against itself
                    const u32x4 si = load_unit(job.a[i] + ao, live, sp) ^ load_unit(job.b[i] + bo, live, sp);
                    const CU32 tp = qtab + (size_t(gi - 1u) * job.k + j0) * 5u;
                    for (uint32_t jj = 0; jj < nj; ++jj) {
                        const Tab t[1] = {tab_at(tp + jj * 5u)};
                        const uint32_t d = (si.x ^ gf_dot<1>(t, z[0])) | (si.y ^ gf_dot<1>(t, z[1])) |
                                           (si.z ^ gf_dot<1>(t, z[2])) | (si.w ^ gf_dot<1>(t, z[3]));
                        if (__builtin_amdgcn_ballot_w64(d != 0u) != 0ull) excl |= 1u << jj;
                    }
                }
                if (excl != 0u && lane == 0u) mismatch_or(base, job.xbit + j0, excl);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// locate_finish: one lane per stripe turns the stripe's working words into its
// verdict (include/zfec_hip.h, fec_locate_batch): no mismatch bit -> CLEAN; one
// check only -> UNKNOWN; exactly one mismatch bit -> that check's slot; exactly
// one basis slot not excluded -> that slot; else MANY.  A plain vector store.
// ---------------------------------------------------------------------------
constexpr uint32_t kLocateClean = 0xFFFFFFFFu, kLocateMany = 0xFFFFFFFEu, kLocateUnknown = 0xFFFFFFFDu;

struct alignas(16) FinishJob {
    const uint32_t* bits;
    uint32_t* culprit;
    uint32_t nstripes, k, c, words;
};

__device__ __forceinline__ uint32_t low_bits(uint32_t n) { return n >= 32u ? 0xFFFFFFFFu : (1u << n) - 1u; }

// The verdict of one stripe's working words `w` (rules 1-5).
__device__ __forceinline__ uint32_t finish_verdict(const uint32_t* w, uint32_t k, uint32_t c) {
    const uint32_t cw = (c + 31u) / 32u, kw = (k + 31u) / 32u;
    uint32_t nbad = 0, first = 0;
    for (uint32_t i = 0; i < cw; ++i) {
        const uint32_t v = w[i] & low_bits(c - 32u * i);
        if (v != 0u && nbad == 0u) first = 32u * i + static_cast<uint32_t>(__builtin_ctz(v));
        nbad += static_cast<uint32_t>(__builtin_popcount(v));
    }
    if (nbad == 0u) return kLocateClean;
    if (c == 1u) return kLocateUnknown;
    if (nbad == 1u) return k + first;
    uint32_t nleft = 0, slot = 0;
    for (uint32_t i = 0; i < kw; ++i) {
        const uint32_t v = ~w[cw + i] & low_bits(k - 32u * i);
        if (v != 0u && nleft == 0u) slot = 32u * i + static_cast<uint32_t>(__builtin_ctz(v));
        nleft += static_cast<uint32_t>(__builtin_popcount(v));
    }
    return nleft == 1u ? slot : kLocateMany;
}

__global__ __launch_bounds__(kBlock) void locate_finish(const FinishJob job) {
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= job.nstripes) return;
    job.culprit[s] = finish_verdict(job.bits + size_t(s) * job.words, job.k, job.c);
}

// ---------------------------------------------------------------------------
// matverify_ragged<K, R> / matlocate_ragged<K, R>: the scrub of a batch whose
// stripes each have their own size (fec_verify_batch_ragged /
// fec_locate_batch_ragged), k <= 4 and up to 8 checks per launch.  One body,
// LOC choosing the family: ragged_walk around the unit of matverify_reg /
// matlocate_reg (the syndromes in registers, the tail zero-filled on both
// sides; with LOC the k hypotheses against the Q tables, read through the
// kernel-argument pointer under the wave-uniform mask != 0 branch only).
//
// There is ONE base pointer: slot j of a stripe is base + off + j * B, so the
// first check slot of a launch (K + bit0) is a number, not a pointer array.
//
// A wave walks several units of one stripe and several stripes in one range,
// so mismatch and excluded bits are accumulated per (wave, stripe) in two
// wave-uniform words, reset at every stripe boundary.  One lane ORs them into
// the stripe's words once, when the wave leaves the stripe, and only if they
// are nonzero: clean data performs no store and no atomic.  A stripe that
// does not fit, or has no bytes, is not read and contributes no bit.  The
// verdict of a stripe is formed after the launch from the OR over all waves
// (locate_finish), never per wave: two waves that each saw another single
// corrupt slot leave both slots' rivals excluded, which is MANY.
// ---------------------------------------------------------------------------
template <int K, int R, bool LOC>
struct alignas(16) RaggedScrubJob {
    uint64_t bstride;  // 0: the stripe's own size (packed objects)
    uint64_t bytes;    // extent of the arena
    uint32_t nstripes;
    uint32_t slots;  // blocks per stripe of the whole call (the fit test)
    uint32_t chk0;   // slot of this launch's first check row
    uint32_t bit0;   // its bit index
    uint32_t words;  // result (verify) or working (locate) words per stripe
    uint32_t xbit;   // bit index of basis slot 0's excluded bit (locate)
    const uint64_t* ustart;  // nstripes + 1
    const uint64_t* sizes;
    const uint64_t* off;
    const uint8_t* src;
    uint32_t* bits;
    uint32_t tab[K * R * 5];                       // row i, input j at (i*K + j)*5
    uint32_t qtab[LOC ? K * (R - 1) * 5 : 1];      // Q[r][j], r = 1..R-1, at ((r-1)*K + j)*5
};

template <int K, int R, bool LOC>
__device__ __forceinline__ void scrub_ragged_body(const RaggedScrubJob<K, R, LOC>& job) {
    using J = RaggedScrubJob<K, R, LOC>;
    // as matapply_ragged: the walk's wave-uniform state leaves few SGPRs, so each
    // row's tables are read where they are used from a lower threshold on
    // (matlocate_ragged<1,2> spilled three with its tables held)
    constexpr bool AL = K * R * 5 >= (LOC ? 10 : 15);
    Tab T[R][K];
    if constexpr (!AL) {
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const uint32_t* t = &job.tab[(r * K + j) * 5];
                T[r][j] = Tab{t[0], t[1], t[2], t[3], t[4]};
            }
    }
    const uint32_t lane = threadIdx.x & 63u;
    const RaggedDesc<1, false> desc{job.nstripes, job.ustart, job.sizes, {job.off}, nullptr};
    ragged_walk(desc, [&](const RaggedStripe<1, false>& cur, uint32_t s, uint64_t u, uint64_t stop) {
        const uint64_t sz = cur.sz;
        const uint64_t B = job.bstride ? job.bstride : sz;
        uint32_t smask = 0, sexcl = 0;  // this wave's bits of stripe s
        if (u < stop && ragged_fits(cur.off[0], B, job.slots, sz, job.bytes)) {
            const uint8_t* const in0 = job.src + cur.off[0];
            const uint64_t coff = job.chk0 * B;
            for (uint64_t w = u - cur.u0, we = stop - cur.u0; w < we; ++w) {
                bool live;
                const Span sp = ragged_unit(w, lane, sz, &live);
                // the K basis rows, then the R stored check rows from slot chk0 on
                u32x4 x[K], y[R];
#pragma unroll
                for (int j = 0; j < K; ++j) x[j] = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
                for (int r = 0; r < R; ++r) y[r] = u32x4{0u, 0u, 0u, 0u};
                if (live) {
                    // the row address advances per lane, as matapply_ragged's output rows do
                    const uint8_t* row = in0 + sp.off;
                    const uint8_t* crow = row + coff;
                    if (sp.full) {
#pragma unroll
                        for (int j = 0; j < K; ++j, row = next_row(row, B)) x[j] = load16(row);
#pragma unroll
                        for (int r = 0; r < R; ++r, crow = next_row(crow, B)) y[r] = load16(crow);
                    } else {
#pragma unroll
                        for (int j = 0; j < K; ++j, row = next_row(row, B)) x[j] = load_tail(row, sp.nb);
#pragma unroll
                        for (int r = 0; r < R; ++r, crow = next_row(crow, B)) y[r] = load_tail(crow, sp.nb);
                    }
                }
                Sel sel[4][K];
                if constexpr (LOC) {
                    unit_sel<K>(sel, x);
                } else {
                    // written out: through unit_sel matverify_ragged<4,3> and <4,7> take two VGPRs
                    // more and lose a wave per SIMD
#pragma unroll
                    for (int j = 0; j < K; ++j) {
                        sel[0][j] = selectors(x[j].x);
                        sel[1][j] = selectors(x[j].y);
                        sel[2][j] = selectors(x[j].z);
                        sel[3][j] = selectors(x[j].w);
                    }
                }
                uint32_t mask = 0;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    Tab t[K];
                    if constexpr (AL) {
                        // the pointer is formed after the previous row's ballot (mask), so at
                        // most two rows' tables are in SGPRs at a time: left free, the
                        // scheduler requests several rows at once and the walk's state spills
                        KPtr<J> kj = kernarg_job<J>();
                        asm volatile("" : "+s"(kj) : "s"(mask));
#pragma unroll
                        for (int j = 0; j < K; ++j) {
                            const uint32_t i = (r * K + j) * 5;
                            t[j] = Tab{kj->tab[i], kj->tab[i + 1], kj->tab[i + 2], kj->tab[i + 3], kj->tab[i + 4]};
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < K; ++j) t[j] = T[r][j];
                    }
                    // the syndrome of row r replaces the stored row
                    y[r].x ^= gf_dot<K>(t, sel[0]);
                    y[r].y ^= gf_dot<K>(t, sel[1]);
                    y[r].z ^= gf_dot<K>(t, sel[2]);
                    y[r].w ^= gf_dot<K>(t, sel[3]);
                    const uint32_t d = y[r].x | y[r].y | y[r].z | y[r].w;
                    if (__builtin_amdgcn_ballot_w64(d != 0u) != 0ull) mask |= 1u << r;
                }
                smask |= mask;
                if constexpr (LOC) {
                    if (mask != 0u) {  // wave-uniform: a scalar branch, not taken on clean data
                        const Sel z[4][1] = {
                            {selectors(y[0].x)}, {selectors(y[0].y)}, {selectors(y[0].z)}, {selectors(y[0].w)}};
#pragma unroll
                        for (int j = 0; j < K; ++j) {
                            uint32_t d = 0;
#pragma unroll
                            for (int r = 1; r < R; ++r) {
                                const KPtr<J> kj = kernarg_job<J>();
                                const uint32_t i = ((r - 1) * K + j) * 5;
                                const Tab qt[1] = {Tab{kj->qtab[i], kj->qtab[i + 1], kj->qtab[i + 2], kj->qtab[i + 3],
                                                       kj->qtab[i + 4]}};
                                d |= (y[r].x ^ gf_dot<1>(qt, z[0])) | (y[r].y ^ gf_dot<1>(qt, z[1])) |
                                     (y[r].z ^ gf_dot<1>(qt, z[2])) | (y[r].w ^ gf_dot<1>(qt, z[3]));
                            }
                            if (__builtin_amdgcn_ballot_w64(d != 0u) != 0ull) sexcl |= 1u << j;
                        }
                    }
                }
            }
        }
        // leaving stripe s: its bits go out once per (wave, stripe)
        if ((smask | sexcl) != 0u && lane == 0u) {
            uint32_t* const base = job.bits + size_t(s) * job.words;
            if (smask != 0u) mismatch_or(base, job.bit0, smask);
            if (LOC && sexcl != 0u) mismatch_or(base, job.xbit, sexcl);
        }
    });
}

template <int K, int R>
__global__ __launch_bounds__(kBlock) void matverify_ragged(const RaggedScrubJob<K, R, false> job) {
    scrub_ragged_body<K, R, false>(job);
}

template <int K, int R>
__global__ __launch_bounds__(kBlock) void matlocate_ragged(const RaggedScrubJob<K, R, true> job) {
    scrub_ragged_body<K, R, true>(job);
}

// ---------------------------------------------------------------------------
// ragged_unfit: the marks of a ragged scrub whose descriptor arrays are device
// memory.  One lane per stripe tests the fit (a size past the arena, which
// ragged_scan gave no units, fails it too) and marks a nonempty stripe that
// does not fit, which the block kernel did not read: all c check bits
// (verify: a scrub must not vouch for what it did not read) or, with c == 0,
// the verdict FEC_LOCATE_UNFIT.  Plain vector stores.
// ---------------------------------------------------------------------------
constexpr uint32_t kLocateUnfit = 0xFFFFFFFBu;

struct alignas(16) UnfitJob {
    const uint64_t* sizes;
    const uint64_t* off;
    uint64_t bstride, bytes;
    uint32_t* out;
    uint32_t nstripes, slots, words, c;
};

__global__ __launch_bounds__(kBlock) void ragged_unfit(const UnfitJob job) {
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= job.nstripes) return;
    const uint64_t sz = job.sizes[s];
    if (sz == 0 || ragged_fits(job.off[s], job.bstride ? job.bstride : sz, job.slots, sz, job.bytes)) return;
    if (job.c == 0u) {
        job.out[s] = kLocateUnfit;
        return;
    }
    for (uint32_t i = 0; i < job.words; ++i) job.out[size_t(s) * job.words + i] = low_bits(job.c - 32u * i);
}

// ---------------------------------------------------------------------------
// matcorrect_reg<K> / rows_correct: in-place correction (fec_correct_batch)
// over the verdict words locate_finish wrote.  The walk is WaveWalk
// (a wave's 64 units lie in ONE stripe), but the stripe's verdict h is read
// FIRST, wave-uniform through a constant-address-space pointer: a verdict >=
// nb (CLEAN, MANY, UNKNOWN) takes a scalar branch around everything, so a
// clean stripe costs one scalar load per wave and no vector memory
// instruction (almost every stripe is clean; loading before the verdict is
// known would read the whole batch a second time).
//
// For a slot verdict h the sources and the target are chosen per stripe by
// wave-uniform address arithmetic: slot j sits at blocks + j * bstride, source
// l is slot (l == h ? k : l) -- check 0 stands in for a bad basis slot, and for
// h >= k no l equals h -- and the target is slot h.  Record h of the uploaded
// tables (k coefficients, the Tab layout) is row h of fec_correct_rows; it comes
// by scalar loads, so v_perm takes the tables as SGPR pairs.  The target is
// never among its own sources: rewriting it in place has no read/write hazard,
// and the overlapped last chunk's two lanes store identical bytes.
//
// matcorrect_reg<K> (k = K <= 4): K loads, gf_dot<K>, one streaming store (byte
// by byte for a block shorter than a chunk, so no byte past sz is written).
// rows_correct (any k): a loop over the k sources, each coefficient's table by
// wave-uniform scalar loads, the result accumulated in registers.  Dirty
// stripes are rare; its speed is not a goal.
// ---------------------------------------------------------------------------
struct alignas(16) CorrectJob {
    Walk walk;
    uint64_t bstride, sstride;
    uint32_t k, nb;
    const uint32_t* tabs;     // nb records of k * 5 dwords
    const uint32_t* verdict;  // nstripes verdict words
    uint8_t* blocks;          // slot 0 of the launch's first stripe (and byte range)
};

template <int K>
__global__ __launch_bounds__(kBlock) void matcorrect_reg(const CorrectJob job) {
    const uint32_t lane = threadIdx.x & 63u;
    const CU32 verdict = (CU32)job.verdict;
    for (WaveWalk it(job.walk, grid_wave()); it.s < job.walk.nstripes; it.next(job.walk)) {
        const uint32_t h = __builtin_amdgcn_readfirstlane(verdict[it.s]);
        if (h < job.nb) {  // wave-uniform: a scalar branch, not taken on clean data
            bool live;
            const Span sp = wave_unit(job.walk, it.w, lane, &live);
            uint8_t* const base = job.blocks + it.s * job.sstride + sp.off;
            u32x4 x[K];
#pragma unroll
            for (int l = 0; l < K; ++l) {
                const uint32_t slot = static_cast<uint32_t>(l) == h ? static_cast<uint32_t>(K) : static_cast<uint32_t>(l);
                x[l] = load_unit(base + slot * job.bstride, live, sp);
            }
            Tab t[K];
            row_tabs<K>(t, (CU32)job.tabs + size_t(h) * (K * 5));
            Sel sel[4][K];
            unit_sel<K>(sel, x);
            const u32x4 y{gf_dot<K>(t, sel[0]), gf_dot<K>(t, sel[1]), gf_dot<K>(t, sel[2]), gf_dot<K>(t, sel[3])};
            store_unit(base + h * job.bstride, y, live, sp);
        }
    }
}

__global__ __launch_bounds__(kBlock) void rows_correct(const CorrectJob job) {
    const uint32_t lane = threadIdx.x & 63u;
    const CU32 verdict = (CU32)job.verdict;
    for (WaveWalk it(job.walk, grid_wave()); it.s < job.walk.nstripes; it.next(job.walk)) {
        const uint32_t h = __builtin_amdgcn_readfirstlane(verdict[it.s]);
        if (h < job.nb) {  // wave-uniform
            bool live;
            const Span sp = wave_unit(job.walk, it.w, lane, &live);
            uint8_t* const base = job.blocks + it.s * job.sstride + sp.off;
            const CU32 tp = (CU32)job.tabs + size_t(h) * job.k * 5u;
            u32x4 y{0u, 0u, 0u, 0u};
            for (uint32_t l = 0; l < job.k; ++l) {
                const uint32_t slot = l == h ? job.k : l;
                const u32x4 x = load_unit(base + slot * job.bstride, live, sp);
                const Tab t[1] = {tab_at(tp + l * 5u)};
                const Sel z[4][1] = {{selectors(x.x)}, {selectors(x.y)}, {selectors(x.z)}, {selectors(x.w)}};
                y.x ^= gf_dot<1>(t, z[0]);
                y.y ^= gf_dot<1>(t, z[1]);
                y.z ^= gf_dot<1>(t, z[2]);
                y.w ^= gf_dot<1>(t, z[3]);
            }
            store_unit(base + h * job.bstride, y, live, sp);
        }
    }
}

// ---------------------------------------------------------------------------
// matrepair_ragged<K, R>: a batched repair whose stripes each have their own
// size AND their own pattern (fec_repair_batch_ragged), k <= 4 and up to 8
// output rows per launch: ragged_walk, the stripe's pattern id its extra word,
// with matapply_ragged's fit test on both arenas (over ALL the call's rows,
// stored or not).
//
// The per-stripe matrix is matrepair_mixed's: the stripe's pattern id is read
// with its descriptor and formed through readfirstlane, so the record address
// and the live-row mask are wave-uniform; each live row's tables come by scalar
// loads where they are used (the empty asm on the record pointer keeps at most
// two rows' tables in SGPRs), and a row whose mask bit is clear is a scalar
// branch around load, arithmetic and store.  The record layout is
// repair_fill_records', unchanged.  An id >= npatterns, a stripe that does not
// fit, or one none of whose rows in this launch is live is neither read nor
// written.
//
// A wave's range crosses stripes: id, record pointer and mask are formed anew
// at every stripe boundary, inside the stripe's own scope -- nothing carries
// from one stripe to the next.  Stores are store16_pol<0> and store_tail,
// plain vector stores.  Records, ids and descriptors are written before the
// launch (a copy, ragged_scan or the caller's earlier work in the stream),
// never by this kernel, so the scalar reads are coherent.
// ---------------------------------------------------------------------------
struct alignas(16) RaggedRepairJob {
    uint64_t in_bstride, out_bstride;  // 0: the stripe's own size (packed objects)
    uint64_t in_bytes, out_bytes;      // extents of the two arenas
    uint32_t nstripes;
    uint32_t rows_all;  // targets per stripe of the whole call (the fit test)
    uint32_t row0;      // this launch takes rows row0 .. row0 + R: its first mask bit
    uint32_t npatterns;
    uint32_t rec_dwords;  // dwords per pattern record
    uint32_t tab_off;     // dword offset in a record of this launch's first row
    uint32_t mask_off;    // dword offset in a record of the live-row mask
    uint32_t pad_;
    const uint64_t* ustart;  // nstripes + 1
    const uint64_t* sizes;
    const uint64_t* in_off;
    const uint64_t* out_off;
    const uint32_t* records;  // npatterns x rec_dwords
    const uint32_t* ids;      // nstripes pattern ids
    const uint8_t* in;
    uint8_t* out;
};

template <int K, int R>
__global__ __launch_bounds__(kBlock) void matrepair_ragged(const RaggedRepairJob job) {
    const uint32_t lane = threadIdx.x & 63u;
    const RaggedDesc<2, true> desc{job.nstripes, job.ustart, job.sizes, {job.in_off, job.out_off}, job.ids};
    ragged_walk(desc, [&](const RaggedStripe<2, true>& cur, uint32_t, uint64_t u, uint64_t stop) {
        const uint64_t sz = cur.sz;
        const uint64_t ib = job.in_bstride ? job.in_bstride : sz, ob = job.out_bstride ? job.out_bstride : sz;
        const uint32_t id = __builtin_amdgcn_readfirstlane(cur.word);
        // the launch's record geometry is read from the argument segment where a stripe needs
        // it, not kept in SGPRs across the walk
        const KPtr<RaggedRepairJob> kj = kernarg_job<RaggedRepairJob>();
        if (u < stop && id < kj->npatterns && ragged_fits(cur.off[0], ib, K, sz, job.in_bytes) &&
            ragged_fits(cur.off[1], ob, job.rows_all, sz, job.out_bytes)) {
            // this stripe's record, mask and table pointer: formed here, dead at the closing brace
            const CU32 rp = (CU32)kj->records + size_t(id) * kj->rec_dwords;
            const uint32_t row0 = kj->row0;
            const uint32_t smask = (__builtin_amdgcn_readfirstlane(rp[kj->mask_off]) >> row0) & ((1u << R) - 1u);
            if (smask != 0u) {  // wave-uniform: a stripe with no live row here is not read
                CU32 tp = rp + kj->tab_off;
                // and the arenas' bases, as matapply_ragged's (<4,2> and up: 8 spills where their own
                // walk had 6)
                const uint8_t* const in0 = kj->in + cur.off[0];
                uint8_t* const out0 = kj->out + cur.off[1] + row0 * ob;
                for (uint64_t w = u - cur.u0, we = stop - cur.u0; w < we; ++w) {
                    // opaque per unit: the R row tests stay bit tests of one SGPR here; hoisted
                    // out of the unit loop each would live in an SGPR pair of its own
                    uint32_t mask = smask;
                    asm volatile("" : "+s"(mask));
                    bool live;
                    const Span sp = ragged_unit(w, lane, sz, &live);
                    // the slot address advances per lane (next_row): the multiples j * ib as
                    // wave-uniform values would live across the unit loop (<4,2> and up re-read
                    // one from a VGPR lane per unit)
                    u32x4 x[K];
#pragma unroll
                    for (int j = 0; j < K; ++j) x[j] = u32x4{0u, 0u, 0u, 0u};
                    if (live) {
                        const uint8_t* row = in0 + sp.off;
                        if (sp.full) {
#pragma unroll
                            for (int j = 0; j < K; ++j, row = next_row(row, ib)) x[j] = load16(row);
                        } else {
#pragma unroll
                            for (int j = 0; j < K; ++j, row = next_row(row, ib)) x[j] = load_tail(row, sp.nb);
                        }
                    }
                    Sel sel[4][K];
                    unit_sel<K>(sel, x);
                    // the row address advances per lane, as matapply_ragged's does
                    uint8_t* orow = out0 + sp.off;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        if ((mask >> r) & 1u) {  // wave-uniform: a scalar branch
                            asm volatile("" : "+s"(tp));
                            Tab t[K];
#pragma unroll
                            for (int j = 0; j < K; ++j) {
                                const uint32_t i = (r * K + j) * 5;
                                t[j] = Tab{tp[i], tp[i + 1], tp[i + 2], tp[i + 3], tp[i + 4]};
                            }
                            const u32x4 y{gf_dot<K>(t, sel[0]), gf_dot<K>(t, sel[1]), gf_dot<K>(t, sel[2]),
                                          gf_dot<K>(t, sel[3])};
                            if (live) {
                                if (sp.full)
                                    store16_pol<0>(orow, y);
                                else
                                    store_tail(orow, y, sp.nb);
                            }
                        }
                        orow += ob;
                    }
                }
            }
        }
    });
}

// ---------------------------------------------------------------------------
// matcorrect_ragged<K>: in-place correction of a batch whose stripes each have
// their own size (fec_correct_batch_ragged), k = K <= 4, over the verdict words
// locate_finish and ragged_unfit wrote earlier in the stream -- never this
// kernel, so the scalar reads of them are coherent.  ragged_walk over the
// ustart the location staged; the stripe's verdict h is its extra word, read
// with its descriptor by a scalar load.  Unless h names a slot AND
// the stripe passes this kernel's own fit test over all nb slots (it does not
// rely on the UNFIT verdict), a scalar branch goes around the whole stripe: a
// clean stripe costs scalar loads and no vector memory instruction.
//
// For a slot verdict the body is matcorrect_reg's: source l is slot
// (l == h ? K : l), record h of the fec_correct_rows tables comes by scalar
// loads, one store per lane (byte by byte below a chunk, so no byte past
// sizes[s] of slot h is written: in a packed object that byte is slot h + 1's
// or the next stripe's).  The target is never among its sources.  Hence a
// stripe split between two waves, and the overlapped last chunk's two lanes,
// write identical bytes and read none that are written: no order between
// them is needed.
// ---------------------------------------------------------------------------
struct alignas(16) RaggedCorrectJob {
    uint64_t bstride;  // 0: the stripe's own size (packed objects)
    uint64_t bytes;    // extent of the arena
    uint32_t nstripes;
    uint32_t nb;  // slots per stripe
    const uint64_t* ustart;  // nstripes + 1
    const uint64_t* sizes;
    const uint64_t* off;
    const uint32_t* tabs;     // nb records of K * 5 dwords
    const uint32_t* verdict;  // nstripes verdict words
    uint8_t* blocks;
};

template <int K>
__global__ __launch_bounds__(kBlock) void matcorrect_ragged(const RaggedCorrectJob job) {
    const uint32_t lane = threadIdx.x & 63u;
    const RaggedDesc<1, true> desc{job.nstripes, job.ustart, job.sizes, {job.off}, job.verdict};
    ragged_walk(desc, [&](const RaggedStripe<1, true>& cur, uint32_t, uint64_t u, uint64_t stop) {
        const uint64_t sz = cur.sz;
        const uint64_t B = job.bstride ? job.bstride : sz;
        const uint32_t h = __builtin_amdgcn_readfirstlane(cur.word);
        // wave-uniform: a scalar branch, not taken on clean data
        if (h < job.nb && u < stop && ragged_fits(cur.off[0], B, job.nb, sz, job.bytes)) {
            // the tables' base is read from the argument segment here, where a dirty stripe needs it
            uint8_t* const base = job.blocks + cur.off[0];
            CU32 tp = (CU32)kernarg_job<RaggedCorrectJob>()->tabs + size_t(h) * (K * 5);
            for (uint64_t w = u - cur.u0, we = stop - cur.u0; w < we; ++w) {
                bool live;
                const Span sp = ragged_unit(w, lane, sz, &live);
                u32x4 x[K];
#pragma unroll
                for (int l = 0; l < K; ++l) {
                    const uint32_t slot =
                        static_cast<uint32_t>(l) == h ? static_cast<uint32_t>(K) : static_cast<uint32_t>(l);
                    x[l] = load_unit(base + slot * B + sp.off, live, sp);
                }
                asm volatile("" : "+s"(tp));  // the tables are read per unit, not held across the walk
                Tab t[K];
#pragma unroll
                for (int l = 0; l < K; ++l)
                    t[l] = Tab{tp[l * 5], tp[l * 5 + 1], tp[l * 5 + 2], tp[l * 5 + 3], tp[l * 5 + 4]};
                Sel sel[4][K];
                unit_sel<K>(sel, x);
                const u32x4 y{gf_dot<K>(t, sel[0]), gf_dot<K>(t, sel[1]), gf_dot<K>(t, sel[2]), gf_dot<K>(t, sel[3])};
                if (live) {
                    uint8_t* const out = base + h * B + sp.off;
                    if (sp.full)
                        store16_pol<0>(out, y);
                    else
                        store_tail(out, y, sp.nb);
                }
            }
        }
    });
}

// ---------------------------------------------------------------------------
// Pair location and correction (fec_locate2_batch / fec_correct2_batch), over
// the stripes the single-block rules call MANY.
//
// locate2_finish: locate_finish's verdicts into plane 0 and NONE into plane 1
// (plain stores).  A MANY stripe, when the pair pass runs (pw != 0), takes the
// next entry of the dirty list -- list[0] is the counter, cleared with the
// working words; a relaxed device-scope fetch_add -- stores its index there
// and clears the entry's pw pair words, so clean data never touches them.
//
// pairs_locate: one wave per workgroup over a grid the host fixes without
// knowing the list's length.  A wave reads the counter by a scalar load first
// and leaves at once on an empty list, else walks (entry, 64-unit wave of the
// stripe) grid-stride.  Per unit the c syndromes are formed in the lane's own
// LDS slots (row i of lane l at (i * 64 + l) * 16 bytes: lanes read only what
// they wrote, so no barrier; rows are addressed at wave-uniform offsets, so no
// dynamically indexed register array exists): the stored checks first, then
// P[i][j] . basis_j accumulated from P's tables by wave-uniform scalar loads.
// A wave whose syndromes are all zero refutes nothing.  Otherwise every pair's
// record is walked: r0, r1 (two rows on which [p_a p_b] has a nonzero minor),
// then c - 2 entries (i, alpha's table, beta's table) with
// s_i ^ alpha . s_r0 ^ beta . s_r1 == 0 at every byte iff the syndrome lies in
// span(p_a, p_b); the first nonzero ballot refutes the pair and ends its walk.
// Refuted bits leave 32 pairs at a time, from one lane, by a relaxed
// device-scope fetch_or into the entry's pair words.
//
// pairs_finish: one lane per list entry; exactly one zero among the first
// npairs pair bits names (a, b), written into both planes by plain stores.
//
// pairs_correct: WaveWalk over the list, as pairs_locate.  A wave reads its entry's
// two verdict words first and touches no block unless they name a pair; then
// record p (k source slots, 2 x k tables) is applied to the sources by
// wave-uniform address arithmetic, and slots a and b take two streaming stores
// per unit (store_tail for a block shorter than a chunk).  The targets are
// never among the sources.  Dirty stripes are rare; speed is not a goal here.
// ---------------------------------------------------------------------------
constexpr uint32_t kLocateNone = 0xFFFFFFFCu;

struct alignas(16) Finish2Job {
    const uint32_t* bits;
    uint32_t* culprit;   // two planes of nstripes words
    uint32_t* list;      // [0] the counter, [1 + e] the stripe of entry e
    uint32_t* pairbits;  // pw words per entry
    uint32_t nstripes, k, c, words;
    uint32_t pw;     // pw == 0: no pair pass
    uint32_t plane;  // words from plane 0 to plane 1 (a run of a ragged call: the whole call's stripes)
    uint32_t pad_[2];
};

__global__ __launch_bounds__(kBlock) void locate2_finish(const Finish2Job job) {
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= job.nstripes) return;
    const uint32_t v = finish_verdict(job.bits + size_t(s) * job.words, job.k, job.c);
    job.culprit[s] = v;
    job.culprit[size_t(job.plane) + s] = kLocateNone;
    if (v == kLocateMany && job.pw != 0u) {
        const uint32_t e = __hip_atomic_fetch_add(job.list, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        job.list[size_t(1) + e] = s;
        uint32_t* const p = job.pairbits + size_t(e) * job.pw;
        for (uint32_t i = 0; i < job.pw; ++i) p[i] = 0u;
    }
}

struct alignas(16) PairsJob {
    Walk walk;               // over list entries: gs_s counts entries
    uint64_t bstride, sstride;
    uint32_t k, c, nb;
    uint32_t npairs, pw;   // pw = ceil(npairs / 32)
    uint32_t plane;        // words from plane 0 to plane 1
    const uint32_t* list;
    uint32_t* pairbits;
    uint32_t* culprit;       // two planes, `plane` words apart
    const uint32_t* ptabs;   // pairs_locate: P's c * k tables (row-major)
    const uint32_t* recs;    // pairs_locate: npairs records of 2 + 11 (c - 2) dwords;
                             // pairs_correct: npairs records of k + 10 k dwords
    uint8_t* blocks;         // slot 0 of stripe 0
};

extern __shared__ u32x4 pairs_syn[];  // c rows of 64 lanes

// One unit of the pair location, for pairs_locate and pairs_locate_ragged
// alike: `base` is this lane's span of slot 0, B the stripe's block stride,
// `words` the entry's pair words.
__device__ __forceinline__ void pairs_locate_unit(const uint8_t* base, uint64_t B, bool live, const Span& sp,
                                                  uint32_t lane, uint32_t k, uint32_t c, uint32_t npairs, CU32 ptabs,
                                                  CU32 recs, uint32_t* words) {
    const uint32_t rec = 2u + 11u * (c - 2u);
    for (uint32_t i = 0; i < c; ++i) pairs_syn[i * 64u + lane] = load_unit(base + (k + i) * B, live, sp);
    for (uint32_t j = 0; j < k; ++j) {
        const u32x4 x = load_unit(base + j * B, live, sp);
        const Sel z[4][1] = {{selectors(x.x)}, {selectors(x.y)}, {selectors(x.z)}, {selectors(x.w)}};
        for (uint32_t i = 0; i < c; ++i) {
            const Tab t[1] = {tab_at(ptabs + (size_t(i) * k + j) * 5u)};
            u32x4 v = pairs_syn[i * 64u + lane];
            v.x ^= gf_dot<1>(t, z[0]);
            v.y ^= gf_dot<1>(t, z[1]);
            v.z ^= gf_dot<1>(t, z[2]);
            v.w ^= gf_dot<1>(t, z[3]);
            pairs_syn[i * 64u + lane] = v;
        }
    }
    uint32_t any = 0;
    for (uint32_t i = 0; i < c; ++i) {
        const u32x4 v = pairs_syn[i * 64u + lane];
        any |= v.x | v.y | v.z | v.w;
    }
    if (__builtin_amdgcn_ballot_w64(any != 0u) != 0ull) {  // wave-uniform
        uint32_t refuted = 0;
        for (uint32_t p = 0; p < npairs; ++p) {
            const CU32 rp = recs + size_t(p) * rec;
            const u32x4 s0 = pairs_syn[rp[0] * 64u + lane], s1 = pairs_syn[rp[1] * 64u + lane];
            const Sel z[4][2] = {{selectors(s0.x), selectors(s1.x)},
                                 {selectors(s0.y), selectors(s1.y)},
                                 {selectors(s0.z), selectors(s1.z)},
                                 {selectors(s0.w), selectors(s1.w)}};
            for (uint32_t m = 0; m + 2u < c; ++m) {
                const CU32 q = rp + 2u + 11u * m;
                const u32x4 si = pairs_syn[q[0] * 64u + lane];
                const Tab t[2] = {tab_at(q + 1), tab_at(q + 6)};
                const uint32_t d = (si.x ^ gf_dot<2>(t, z[0])) | (si.y ^ gf_dot<2>(t, z[1])) |
                                   (si.z ^ gf_dot<2>(t, z[2])) | (si.w ^ gf_dot<2>(t, z[3]));
                if (__builtin_amdgcn_ballot_w64(d != 0u) != 0ull) {
                    refuted |= 1u << (p & 31u);
                    break;
                }
            }
            if ((p & 31u) == 31u || p + 1u == npairs) {
                if (refuted != 0u && lane == 0u)
                    (void)__hip_atomic_fetch_or(words + (p >> 5), refuted, __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_AGENT);
                refuted = 0;
            }
        }
    }
}

__global__ __launch_bounds__(64) void pairs_locate(const PairsJob job) {
    const CU32 list = (CU32)job.list;
    const uint32_t count = list[0];
    WaveWalk it(job.walk, grid_wave<64>());
    if (it.s >= count) return;  // (the empty list: one scalar load)
    const uint32_t lane = threadIdx.x;
    const CU32 ptabs = (CU32)job.ptabs, recs = (CU32)job.recs;
    for (; it.s < count; it.next(job.walk)) {
        const uint32_t e = it.s, s = list[size_t(1) + e];
        bool live;
        const Span sp = wave_unit(job.walk, it.w, lane, &live);
        pairs_locate_unit(job.blocks + s * job.sstride + sp.off, job.bstride, live, sp, lane, job.k, job.c,
                          job.npairs, ptabs, recs, job.pairbits + size_t(e) * job.pw);
    }
}

__global__ __launch_bounds__(kBlock) void pairs_finish(const PairsJob job) {
    const uint32_t count = ((CU32)job.list)[0];
    for (uint64_t e = uint64_t(blockIdx.x) * kBlock + threadIdx.x; e < count; e += uint64_t(gridDim.x) * kBlock) {
        const uint32_t s = job.list[1u + e];
        const uint32_t* const p = job.pairbits + e * job.pw;
        uint32_t nleft = 0, first = 0;
        for (uint32_t i = 0; i < job.pw; ++i) {
            const uint32_t v = ~p[i] & low_bits(job.npairs - 32u * i);
            if (v != 0u && nleft == 0u) first = 32u * i + static_cast<uint32_t>(__builtin_ctz(v));
            nleft += static_cast<uint32_t>(__builtin_popcount(v));
        }
        if (nleft != 1u) continue;  // the planes stay (MANY, NONE)
        // pair index a*nb - a(a+1)/2 + (b - a - 1) back into (a, b)
        uint32_t a = 0, row = job.nb - 1u;
        while (first >= row) {
            first -= row;
            ++a;
            --row;
        }
        job.culprit[s] = a;
        job.culprit[size_t(job.plane) + s] = a + 1u + first;
    }
}

// One unit of the pair correction, for pairs_correct and pairs_correct_ragged
// alike: record rp (k source slots, 2 x k tables) applied at `base`, this
// lane's span of slot 0, B the stripe's block stride.  store_unit writes no
// byte past the block's end.
__device__ __forceinline__ void pairs_correct_unit(uint8_t* base, uint64_t B, bool live, const Span& sp, uint32_t k,
                                                   CU32 rp, uint32_t a, uint32_t b) {
    u32x4 ya{0u, 0u, 0u, 0u}, yb{0u, 0u, 0u, 0u};
    for (uint32_t l = 0; l < k; ++l) {
        const u32x4 x = load_unit(base + rp[l] * B, live, sp);
        const Sel z[4][1] = {{selectors(x.x)}, {selectors(x.y)}, {selectors(x.z)}, {selectors(x.w)}};
        const Tab ta[1] = {tab_at(rp + k + 5u * l)}, tb[1] = {tab_at(rp + 6u * k + 5u * l)};
        ya.x ^= gf_dot<1>(ta, z[0]);
        ya.y ^= gf_dot<1>(ta, z[1]);
        ya.z ^= gf_dot<1>(ta, z[2]);
        ya.w ^= gf_dot<1>(ta, z[3]);
        yb.x ^= gf_dot<1>(tb, z[0]);
        yb.y ^= gf_dot<1>(tb, z[1]);
        yb.z ^= gf_dot<1>(tb, z[2]);
        yb.w ^= gf_dot<1>(tb, z[3]);
    }
    store_unit(base + a * B, ya, live, sp);
    store_unit(base + b * B, yb, live, sp);
}

__global__ __launch_bounds__(kBlock) void pairs_correct(const PairsJob job) {
    const CU32 list = (CU32)job.list;
    const uint32_t count = list[0];
    WaveWalk it(job.walk, grid_wave());
    if (it.s >= count) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t k = job.k;
    const CU32 verdict = (CU32)job.culprit, recs = (CU32)job.recs;
    for (; it.s < count; it.next(job.walk)) {
        const uint32_t s = list[size_t(1) + it.s];
        const uint32_t a = verdict[s], b = verdict[size_t(job.plane) + s];
        if (a < b && b < job.nb) {  // wave-uniform
            bool live;
            const Span sp = wave_unit(job.walk, it.w, lane, &live);
            const uint32_t p = a * job.nb - a * (a + 1u) / 2u + (b - a - 1u);
            pairs_correct_unit(job.blocks + s * job.sstride + sp.off, job.bstride, live, sp, k,
                               recs + size_t(p) * (11u * k), a, b);
        }
    }
}

// ---------------------------------------------------------------------------
// pairs_locate_ragged / pairs_correct_ragged: pairs_locate / pairs_correct over
// the dirty list of a batch whose stripes each have their own size
// (fec_locate2_batch_ragged / fec_correct2_batch_ragged).  The host knows
// neither the list's length nor, with device-side descriptors, any listed
// stripe's size, so it fixes the grid and the waves walk work items
// grid-stride: item i is share i % kPairSplit of entry i / kPairSplit, the
// units j, j + kPairSplit, ... of that entry's stripe.  A short stripe leaves
// its higher shares nothing to do (scalar loads and a scalar branch); a long
// one is spread over kPairSplit waves.  A wave reads the counter by a scalar
// load first and leaves at once on an empty list.  The entry's stripe, and that
// stripe's size and offset, come by scalar loads from the arrays the location
// staged or the caller's device arrays: written before the launch, never by
// these kernels.  The block stride is bstride ? bstride : sizes[s].
//
// Each kernel makes its own fit test over all nb slots (ragged_fits) and does
// not rely on the verdict, as matcorrect_ragged.  Units are ragged_unit's: the
// overlapped last chunk for a block of at least 16 bytes, bytes below a chunk.
// The unit bodies are the uniform kernels' (pairs_locate_unit,
// pairs_correct_unit): the syndromes' LDS layout, c rows of 64 lanes in which
// a lane reads only what it wrote, and the relaxed device-scope fetch_or of
// the refuted pair bits, which here come from several waves and several units
// of one stripe.  pairs_correct_ragged stores through store_unit
// (store16_pol<0> / store_tail): no byte past sizes[s] of slots a and b is
// written.  The targets are never among the sources, so a stripe split between
// waves, and the two lanes of an overlapped chunk, write identical bytes and
// read none that are written: no order between them is needed.
// ---------------------------------------------------------------------------
constexpr uint32_t kPairSplit = 4;

struct alignas(16) PairsRaggedJob {
    uint64_t bstride;   // 0: the stripe's own size (packed objects)
    uint64_t bytes;     // extent of the arena
    uint32_t nstripes;  // also the words from plane 0 to plane 1
    uint32_t k, c, nb;
    uint32_t npairs, pw;
    const uint64_t* sizes;
    const uint64_t* off;
    const uint32_t* list;
    uint32_t* pairbits;
    const uint32_t* culprit;  // pairs_correct_ragged: the two planes
    const uint32_t* ptabs;    // as PairsJob
    const uint32_t* recs;
    uint8_t* blocks;  // the arena
};

__global__ __launch_bounds__(64) void pairs_locate_ragged(const PairsRaggedJob job) {
    const CU32 list = (CU32)job.list;
    const uint64_t items = uint64_t(list[0]) * kPairSplit;
    uint64_t it = blockIdx.x;
    if (it >= items) return;  // (the empty list: one scalar load)
    const uint32_t lane = threadIdx.x;
    const CU32 ptabs = (CU32)job.ptabs, recs = (CU32)job.recs;
    for (; it < items; it += gridDim.x) {
        const uint32_t e = static_cast<uint32_t>(it / kPairSplit), j = static_cast<uint32_t>(it % kPairSplit);
        const uint32_t s = list[size_t(1) + e];
        if (s >= job.nstripes) continue;
        const uint64_t sz = ((CU64)job.sizes)[s], off = ((CU64)job.off)[s];
        const uint64_t B = job.bstride ? job.bstride : sz, nu = ragged_units_of(sz);
        // wave-uniform: a scalar branch
        if (j >= nu || !ragged_fits(off, B, job.nb, sz, job.bytes)) continue;
        const uint8_t* const base = job.blocks + off;
        uint32_t* const words = job.pairbits + size_t(e) * job.pw;
        for (uint64_t w = j; w < nu; w += kPairSplit) {
            bool live;
            const Span sp = ragged_unit(w, lane, sz, &live);
            pairs_locate_unit(base + sp.off, B, live, sp, lane, job.k, job.c, job.npairs, ptabs, recs, words);
        }
    }
}

__global__ __launch_bounds__(kBlock) void pairs_correct_ragged(const PairsRaggedJob job) {
    const CU32 list = (CU32)job.list;
    const uint64_t items = uint64_t(list[0]) * kPairSplit;
    uint64_t it = grid_wave();
    if (it >= items) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t k = job.k;
    const CU32 verdict = (CU32)job.culprit, recs = (CU32)job.recs;
    for (; it < items; it += uint64_t(gridDim.x) * (kBlock / 64)) {
        const uint32_t e = static_cast<uint32_t>(it / kPairSplit), j = static_cast<uint32_t>(it % kPairSplit);
        const uint32_t s = list[size_t(1) + e];
        if (s >= job.nstripes) continue;
        const uint32_t a = verdict[s], b = verdict[size_t(job.nstripes) + s];
        if (!(a < b && b < job.nb)) continue;  // wave-uniform: the planes stayed (MANY, NONE)
        const uint64_t sz = ((CU64)job.sizes)[s], off = ((CU64)job.off)[s];
        const uint64_t B = job.bstride ? job.bstride : sz, nu = ragged_units_of(sz);
        if (j >= nu || !ragged_fits(off, B, job.nb, sz, job.bytes)) continue;
        uint8_t* const base = job.blocks + off;
        const uint32_t p = a * job.nb - a * (a + 1u) / 2u + (b - a - 1u);
        const CU32 rp = recs + size_t(p) * (11u * k);
        for (uint64_t w = j; w < nu; w += kPairSplit) {
            bool live;
            const Span sp = ragged_unit(w, lane, sz, &live);
            pairs_correct_unit(base + sp.off, B, live, sp, k, rp, a, b);
        }
    }
}

// ---------------------------------------------------------------------------
// matapply_lds<ACC, NT, RT>: runtime k and r like matapply_gen, but each
// workgroup first expands its k*r coefficients into LDS tables (32 bytes per
// coefficient).  In the loop a table is two broadcast LDS reads off one base
// address straight into VGPRs, so v_perm_b32 gets all-VGPR operands (gfx9's
// one-SGPR-per-VALU-op limit forces a v_mov per table word pair on the
// scalar path) and no scalar load -> dependent load chain sits in the loop.
// Inputs go in pairs so six partial products share three XOR3s, and rows
// past r in the last tile are skipped by a wave-uniform branch.
// ---------------------------------------------------------------------------
struct LdsTab {
    u32x4 w03;  // c*{0..7} and c*{0,8,..,56}
    u32x4 w4;   // c*{0,64,128,192}, 3 pad words (keeps both reads on one base address)
};

// Entry (input j, row) at j * rp + row, rp >= r: a tile's rows for one input
// are adjacent; rows r..rp-1 (padding up to whole tiles) get the zero table.
__device__ __forceinline__ void lds_tables_build(const MatJob& job, LdsTab* t, uint32_t rp) {
    const uint32_t n = job.k * rp;
    for (uint32_t i = threadIdx.x; i < n; i += kBlock) {
        const uint32_t j = i / rp, row = i - j * rp;
        const uint32_t c = row < job.r ? job.coef[row * job.k + j] : 0u;
        const uint32_t* b = &g_bank.w[c * 8];
        t[i].w03 = u32x4{b[0], b[1], b[2], b[3]};
        t[i].w4 = u32x4{b[4], 0u, 0u, 0u};
    }
    __syncthreads();
}

// acc ^ c0*x0 ^ c1*x1 for four bytes: 6 v_perm_b32 + 3 v_bitop3_b32.
__device__ __forceinline__ uint32_t gf_mac2(uint32_t acc, const u32x4& t0, uint32_t u0, Sel s0, const u32x4& t1,
                                            uint32_t u1, Sel s1) {
    const uint32_t a0 = perm(t0.y, t0.x, s0.s0), b0 = perm(t0.w, t0.z, s0.s1), d0 = perm(u0, u0, s0.s2);
    const uint32_t a1 = perm(t1.y, t1.x, s1.s0), b1 = perm(t1.w, t1.z, s1.s1), d1 = perm(u1, u1, s1.s2);
    return xor3(xor3(xor3(acc, a0, b0), d0, a1), b1, d1);
}

__device__ __forceinline__ uint32_t gf_mac_v(uint32_t acc, const u32x4& t, uint32_t t4, Sel s) {
    const uint32_t a = perm(t.y, t.x, s.s0);
    const uint32_t b = perm(t.w, t.z, s.s1);
    const uint32_t d = perm(t4, t4, s.s2);
    return xor3(xor3(acc, a, b), d, 0u);
}

// D dwords per lane per block (chunk = 4*D bytes): D = 4 is one dwordx4 per
// block, D = 2 halves the accumulator / selector / input registers so more
// waves fit per SIMD.
template <int D>
struct Words {
    uint32_t w[D];
};

template <int D>
__device__ __forceinline__ Words<D> load_words(const uint8_t* p, bool full, uint32_t nb) {
    Words<D> x;
    if (full) {
        __builtin_memcpy(x.w, p, 4 * D);
    } else {
        const u32x4 t = load_tail(p, nb);
        const uint32_t tw[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int v = 0; v < D; ++v) x.w[v] = tw[v];
    }
    return x;
}

template <int D, bool NT>
__device__ __forceinline__ void store_words(uint8_t* p, const Words<D>& y, bool full, uint32_t nb) {
    if (full) {
        if constexpr (D == 4) {
            store16_out<NT>(p, u32x4{y.w[0], y.w[1], y.w[2], y.w[3]});
        } else if constexpr (D == 2) {
            typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
            const u32x2 v{y.w[0], y.w[1]};
            if constexpr (NT)
                __builtin_nontemporal_store(v, reinterpret_cast<u32x2*>(p));
            else
                __builtin_memcpy(p, &v, 8);
        } else {
            __builtin_memcpy(p, y.w, 4 * D);
        }
    } else {
        u32x4 t{0u, 0u, 0u, 0u};
        t.x = y.w[0];
        if constexpr (D > 1) t.y = y.w[1];
        if constexpr (D > 2) t.z = y.w[2];
        if constexpr (D > 3) t.w = y.w[3];
        store_tail(p, t, nb);
    }
}

// One step of the flattened (unit, row tile, input group) walk.
struct Step {
    UnitIter u;
    uint32_t rb, g;
};

// acc[rr] ^= sum over the group's inputs of table(j, rb + rr) * x_j, for the
// RT_ rows of one tile.  FULL: every row of the tile exists (no per-row
// branch, so no register copies where the two paths of a branch meet).
template <bool FULL, int RT_, int D, int GG>
__device__ __forceinline__ void mac_group(uint32_t (&a)[RT_][D], const Words<D> (&x)[GG], const LdsTab* lds_tab,
                                          uint32_t g, uint32_t rb, uint32_t k, uint32_t r) {
#pragma unroll
    for (int jj = 0; jj < GG; jj += 2) {
        const uint32_t j = g + jj;
        if (j >= k) break;
        Sel s0[D];
#pragma unroll
        for (int v = 0; v < D; ++v) s0[v] = selectors(x[jj].w[v]);
        const LdsTab* t0 = lds_tab + j * r + rb;
        if (jj + 1 < GG && j + 1 < k) {  // two inputs: their six partial products share three XOR3s
            Sel s1[D];
#pragma unroll
            for (int v = 0; v < D; ++v) s1[v] = selectors(x[jj + 1].w[v]);
            const LdsTab* t1 = t0 + r;
#pragma unroll
            for (int rr = 0; rr < RT_; ++rr) {
                if (FULL || rb + rr < r) {  // wave-uniform
                    const u32x4 p = t0[rr].w03, q = t1[rr].w03;
                    const uint32_t pu = t0[rr].w4.x, qu = t1[rr].w4.x;
#pragma unroll
                    for (int v = 0; v < D; ++v) a[rr][v] = gf_mac2(a[rr][v], p, pu, s0[v], q, qu, s1[v]);
                }
            }
        } else {
#pragma unroll
            for (int rr = 0; rr < RT_; ++rr) {
                if (FULL || rb + rr < r) {
                    const u32x4 p = t0[rr].w03;
                    const uint32_t pu = t0[rr].w4.x;
#pragma unroll
                    for (int v = 0; v < D; ++v) a[rr][v] = gf_mac_v(a[rr][v], p, pu, s0[v]);
                }
            }
        }
    }
}

// Row tiling of a launch, fixed by the dispatcher:
enum TileMode {
    kTilesRagged = 0,  // rows past r in the last tile are skipped by a per-row branch
    kTilesPadded = 1,  // the table has zero rows up to whole tiles: no branch in the
                       // multiply-accumulate, only the stores of padding rows are skipped
};

// Rows of the LDS table: r, or r rounded up to whole RT-row tiles.
template <int MODE>
__host__ __device__ constexpr uint32_t table_rows(uint32_t r, uint32_t rt) {
    return MODE == kTilesPadded ? (r + rt - 1) / rt * rt : r;
}

template <bool ACC, bool NT, int RT_, int D, int GG, int MODE>
__device__ __forceinline__ void matapply_lds_body(const MatJob& job) {
    constexpr uint32_t CH = 4 * D;
    extern __shared__ LdsTab lds_tab[];
    const uint32_t k = job.k;
    const uint32_t r = job.r;
    const uint32_t rp = table_rows<MODE>(r, RT_);
    lds_tables_build(job, lds_tab, rp);
    const uint64_t sz = job.sz;
    const uint32_t nfull = static_cast<uint32_t>(sz / CH);
    // The walk visits, for each of this lane's units in grid-stride order, each
    // row tile and, inside it, each group of GG inputs.  The loads of the next
    // step's group (possibly the next tile's first group, or the next unit's)
    // are issued before the current group is computed, so a wave never starts
    // a group waiting on HBM.  (rb, g) are wave-uniform; units differ per lane.
    auto load_step = [&](const Step& st, Words<D> (&x)[GG]) {
        const Span sp = chunk_span<CH, !ACC>(st.u.c, sz, nfull);
        const uint64_t ib = st.u.s * job.in_sstride + sp.off;
#pragma unroll
        for (int jj = 0; jj < GG; ++jj)
            if (st.g + jj < k) x[jj] = load_words<D>(job.in[st.g + jj] + ib, sp.full, sp.nb);
    };
    Step cur{UnitIter(job), 0u, 0u};
    bool live = cur.u.s < job.nstripes;
    uint32_t a[RT_][D];
#pragma unroll
    for (int rr = 0; rr < RT_; ++rr)
#pragma unroll
        for (int v = 0; v < D; ++v) a[rr][v] = 0u;
    // One step: prefetch the next step's group into xb, compute the current
    // group from xa, store the tile when its last group is done.  Every lane
    // walks the same (rb, g) sequence; a lane whose units ran out keeps
    // stepping (without memory traffic) until the whole wave is done.
    Words<D> xa[GG];
    if (live) load_step(cur, xa);
    while (__any(live)) {
        // (g, rb) are wave-uniform; say so, or they live in VGPRs and every
        // block pointer becomes a readfirstlane + dependent scalar load.
        cur.g = __builtin_amdgcn_readfirstlane(cur.g);
        cur.rb = __builtin_amdgcn_readfirstlane(cur.rb);
        Step nxt = cur;
        nxt.g += GG;
        const bool tile_end = nxt.g >= k;
        if (tile_end) {
            nxt.g = 0;
            nxt.rb += RT_;
            if (nxt.rb >= r) {
                nxt.rb = 0;
                nxt.u.next(job);
            }
        }
        const bool nlive = nxt.u.s < job.nstripes;
        Words<D> xb[GG];
        if (nlive) load_step(nxt, xb);
        if (live) {
            mac_group<MODE == kTilesPadded, RT_, D, GG>(a, xa, lds_tab, cur.g, cur.rb, k, rp);
            if (tile_end) {
                const Span sp = chunk_span<CH, !ACC>(cur.u.c, sz, nfull);
                const uint64_t ob = cur.u.s * job.out_sstride + sp.off;
#pragma unroll
                for (int rr = 0; rr < RT_; ++rr) {
                    if (cur.rb + rr >= r) continue;  // ragged tail or padding rows
                    uint8_t* op = job.out[cur.rb + rr] + ob;
                    Words<D> y;
#pragma unroll
                    for (int v = 0; v < D; ++v) y.w[v] = a[rr][v];
                    if constexpr (ACC) {
                        const Words<D> o = load_words<D>(op, sp.full, sp.nb);
#pragma unroll
                        for (int v = 0; v < D; ++v) y.w[v] ^= o.w[v];
                    }
                    store_words<D, NT>(op, y, sp.full, sp.nb);
                }
            }
        }
        if (tile_end) {
#pragma unroll
            for (int rr = 0; rr < RT_; ++rr)
#pragma unroll
                for (int v = 0; v < D; ++v) a[rr][v] = 0u;
        }
#pragma unroll
        for (int jj = 0; jj < GG; ++jj) xa[jj] = xb[jj];
        cur = nxt;
        live = nlive;
    }
}

template <bool ACC, bool NT, int RT_, int D, int GG, int MODE = kTilesRagged>
__global__ __launch_bounds__(kBlock) void matapply_lds(const MatJob job) {
    matapply_lds_body<ACC, NT, RT_, D, GG, MODE>(job);
}

// ---------------------------------------------------------------------------
// matapply_bsg<RT, TBL>: bit-sliced, with the coefficient matrix as run-time
// data (no compile step: every erasure pattern runs at this speed the first
// time).
//
// Multiplication by c is an 8x8 GF(2) matrix on the bits of a byte.  After an
// 8x8 bit transpose a lane's 32 bytes are 8 bit-planes p0..p7, and output
// plane b of c*x is L[ml_b] ^ H[mh_b], where L[m] is the XOR of the planes
// {a < 4 : bit a of m} and H[m] that of {4 + a : bit a of m}; ml_b / mh_b are
// the low / high nibble of the bit-b row of c's matrix (bitslice.cpp's JIT
// bakes the same choice of combinations into the instruction stream).  Here
// each input's 15 + 15 combinations go to LDS, and a wave selects them with
// the nibbles as wave-uniform LDS offsets: per coefficient and output plane two
// ds_read_b64 (both of the lane's 32-byte groups at once) and one v_bitop3
// XOR3 per group, against 4.5 VOP3 per 4 bytes for the table kernels.
//
// One workgroup (4 waves) per unit of 4 KiB of every block of a stripe: lane l
// owns bytes 16l + 1024h (h = 0..3) of each block, two 32-byte groups (h = 0,1
// and h = 2,3).  The r output rows are split over the 4 waves (RT rows each,
// accumulators in registers).  Inputs go in phases of 2: waves 0 and 1 each
// load one input of the phase, transpose it and write its combinations to
// their LDS slot; after a barrier every wave folds the phase's 2 inputs into
// its rows.  LDS per slot: 32 combinations x 64 lanes x 8 B = 16 KiB (entries
// 0 and 16 hold zeros, written once).  (Measured and not kept, DESIGN.md §4:
// 4 inputs per phase, a scheduling barrier per row, the input build balanced
// over all 4 waves.)
//
// TBL = false: block pointers and coefficients in the MatJob kernel arguments
// (k <= 32).  TBL = true: in a device-side table the host fills per launch
// (BsgTblJob::table: k input pointers, r output pointers, then the
// coefficients in walk order), read with scalar loads -- k up to 256 in one
// pass, instead of XOR-accumulating passes of 32 inputs.
// ---------------------------------------------------------------------------
constexpr uint32_t kBsgChunk = 4096;        // bytes of each block per unit
constexpr uint32_t kBsgSlotBytes = 32 * 512;  // one input's combinations
constexpr int kBsgPhase = 2;                // inputs per LDS phase

// g_bsg.off[c]: sixteen dwords, the LDS byte offsets of the combinations
// output plane b of c*x needs: [b] = L[ml_b], [8 + b] = H[mh_b] (b = 0..7).
struct BsgBank {
    uint32_t off[256 * 16];
};

constexpr BsgBank make_bsg_bank() {
    BsgBank t{};
    for (uint32_t c = 0; c < 256; ++c) {
        uint32_t p[8] = {};
        p[0] = c;  // c * 2^a
        for (int a = 1; a < 8; ++a) p[a] = ct_xtime(p[a - 1]);
        for (uint32_t b = 0; b < 8; ++b) {
            uint32_t ml = 0, mh = 0;
            for (uint32_t a = 0; a < 4; ++a) {
                ml |= ((p[a] >> b) & 1u) << a;
                mh |= ((p[a + 4] >> b) & 1u) << a;
            }
            t.off[c * 16 + b] = ml * 512u;
            t.off[c * 16 + 8 + b] = (16u + mh) * 512u;
        }
    }
    return t;
}

__constant__ BsgBank g_bsg = make_bsg_bank();

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t bsel(uint32_t m, uint32_t a, uint32_t b) {
    return __builtin_amdgcn_bitop3_b32(a, b, m, 0xE4);  // m ? a : b, bitwise
}

// one block swap of the 8x8 bit transpose, four byte lanes at once
__device__ __forceinline__ void bswap_blocks(uint32_t& a, uint32_t& b, int s, uint32_t m) {
    const uint32_t t0 = bsel(m, a, b << s);
    const uint32_t t1 = bsel(m, a >> s, b);
    a = t0;
    b = t1;
}

// Two block swaps with the same shift at once: the shifts on 64-bit register
// pairs (v_lshlrev_b64 / v_lshrrev_b64 move two dwords at the issue cost of one
// 32-bit shift, profiles/r02_mb_valu.log); the bits crossing the dword boundary
// land where the swap's mask discards them.  Inline asm, or the compiler splits
// the right shift back into v_alignbit + v_lshrrev.  (a0, a1) and (b0, b1) are
// adjacent registers in the first two stages of transpose8 (the 16-byte loads
// and the accumulator rows are register quads), so forming the pairs costs no
// moves.  Same form as bitslice.cpp's sw2.
__device__ __forceinline__ uint64_t vshl64(uint64_t x, int s) {
    uint64_t r;
    asm("v_lshlrev_b64 %0, %1, %2" : "=v"(r) : "i"(s), "v"(x));
    return r;
}
__device__ __forceinline__ uint64_t vshr64(uint64_t x, int s) {
    uint64_t r;
    asm("v_lshrrev_b64 %0, %1, %2" : "=v"(r) : "i"(s), "v"(x));
    return r;
}
__device__ __forceinline__ void bswap_blocks2(uint32_t& a0, uint32_t& b0, uint32_t& a1, uint32_t& b1, int s,
                                              uint32_t m) {
    const uint64_t bl = vshl64((static_cast<uint64_t>(b1) << 32) | b0, s);
    const uint64_t ar = vshr64((static_cast<uint64_t>(a1) << 32) | a0, s);
    const uint32_t t0 = bsel(m, a0, static_cast<uint32_t>(bl)), t1 = bsel(m, static_cast<uint32_t>(ar), b0);
    const uint32_t t2 = bsel(m, a1, static_cast<uint32_t>(bl >> 32)), t3 = bsel(m, static_cast<uint32_t>(ar >> 32), b1);
    a0 = t0;
    b0 = t1;
    a1 = t2;
    b1 = t3;
}

// 8 dwords (32 bytes) <-> 8 bit-planes; the transpose is its own inverse.
// The first two stages run on 64-bit shift pairs, 40 VOP3 instructions instead
// of 48 (tools/ab_bsr.sh, profiles/r06_bsr_ab.json).
__device__ __forceinline__ void transpose8(uint32_t (&v)[8]) {
    bswap_blocks2(v[0], v[4], v[1], v[5], 4, 0x0F0F0F0Fu);
    bswap_blocks2(v[2], v[6], v[3], v[7], 4, 0x0F0F0F0Fu);
    bswap_blocks2(v[0], v[2], v[1], v[3], 2, 0x33333333u);
    bswap_blocks2(v[4], v[6], v[5], v[7], 2, 0x33333333u);
    bswap_blocks(v[0], v[1], 1, 0x55555555u);
    bswap_blocks(v[2], v[3], 1, 0x55555555u);
    bswap_blocks(v[4], v[5], 1, 0x55555555u);
    bswap_blocks(v[6], v[7], 1, 0x55555555u);
}

// The 15 nonzero combinations of planes q[0..3] of both groups, to LDS
// entries base + 1..15 (entry e of lane l at e * 512 + l * 8).
__device__ __forceinline__ void write_combos(char* slot, uint32_t lane8, const uint32_t (&q0)[4],
                                             const uint32_t (&q1)[4], uint32_t base) {
    uint32_t c0[16], c1[16];
    c0[0] = 0u;
    c1[0] = 0u;
#pragma unroll
    for (int m = 1; m < 16; ++m) {
        const int top = 31 - __builtin_clz(m);
        c0[m] = c0[m ^ (1 << top)] ^ q0[top];
        c1[m] = c1[m ^ (1 << top)] ^ q1[top];
        *reinterpret_cast<u32x2*>(slot + (base + m) * 512u + lane8) = u32x2{c0[m], c1[m]};
    }
}

// Rows are interleaved over the waves: wave w owns rows w + 4*rr, rr < RT.
// launch_bsg lays the coefficients out for this walk: wave w's bytes of phase
// f are (js, rr) in order, js < 2, rr < RT, at byte (w * nphases + f) *
// bsg_phase_bytes(RT) (rows past r and inputs past k get coefficient 0,
// whose combinations are the zero entries).  A coefficient's eight offset
// dwords come from g_bsg by scalar loads, issued one step (row) ahead: a wait
// for a scalar load also drains the wave's LDS reads, so it must come where
// the wave has none outstanding.
template <int RT>
__host__ __device__ constexpr uint32_t bsg_phase_bytes() {
    return (kBsgPhase * RT + 3) / 4 * 4;
}

struct alignas(16) BsgTblJob {
    uint64_t sz, in_sstride, out_sstride;
    uint32_t nstripes, k, r, cps, gs_c, gs_s;
    uint32_t ngroups;  // row groups of 4 * RT rows: workgroup units are (group, stripe, unit) triples
    uint32_t pad_;
    const uint8_t* table;  // device memory: k input pointers, r output pointers, per group the walk-order coefficients
};

typedef const __attribute__((address_space(4))) uint64_t* CU64;
typedef const __attribute__((address_space(4))) uint32_t* KWords;

// Block pointers and coefficient words of a launch: from the kernel arguments
// (MatJob, one row group) or from the device-side table (scalar loads either way).
struct BsgKarg {
    KPtr<MatJob> kj;
    __device__ const uint8_t* in(uint32_t j) const { return kj->in[j]; }
    __device__ uint8_t* out(uint32_t i) const { return kj->out[i]; }
    __device__ KWords coef() const { return (KWords)kj->coef; }
};

struct BsgTbl {
    CU64 tp;
    uint32_t k, r;
    __device__ const uint8_t* in(uint32_t j) const { return reinterpret_cast<const uint8_t*>(tp[j]); }
    __device__ uint8_t* out(uint32_t i) const { return reinterpret_cast<uint8_t*>(tp[k + i]); }
    __device__ KWords coef() const { return (KWords)(tp + k + r); }
};

template <int RT, bool TBL, class J>
__global__ __launch_bounds__(256) void matapply_bsg(const J job) {
    constexpr int P = kBsgPhase;
    constexpr uint32_t PB = bsg_phase_bytes<RT>();
    constexpr int ND = PB / 4;           // coefficient dwords per wave and phase
    extern __shared__ char bsg_lds[];    // P slots of kBsgSlotBytes
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t lane8 = lane * 8u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t k = job.k, r = job.r;
    const uint32_t nph = (k + P - 1) / P;
    // zero entries L[0] and H[0] of every slot (never overwritten)
    for (uint32_t i = threadIdx.x; i < P * 2 * 64; i += 256) {
        const uint32_t sl = i / 128, e = (i / 64) & 1u, l = i & 63u;
        *reinterpret_cast<u32x2*>(bsg_lds + sl * kBsgSlotBytes + e * 16u * 512u + l * 8u) = u32x2{0u, 0u};
    }
    const auto src = [&] {
        if constexpr (TBL)
            return BsgTbl{(CU64)job.table, k, r};
        else
            return BsgKarg{kernarg_job<MatJob>()};
    }();
    // The walk's "stripes" are (row group, stripe) pairs, group-major (one group
    // without the table): a launch with few units of work per row group still
    // fills the chip, each workgroup building the combinations of its unit's
    // inputs for its group's rows.
    const uint32_t ns = job.nstripes;
    uint32_t nvs = ns;
    if constexpr (TBL) nvs = ns * job.ngroups;
    const uint32_t rpg = 4u * static_cast<uint32_t>(RT);  // rows per group
    const uint64_t sz = job.sz;
    // byte offset of unit c in a block: the last unit of a block ends at sz
    // (overlapping its neighbour)
    auto unit_off = [&](uint32_t cu) {
        uint64_t o = static_cast<uint64_t>(cu) * kBsgChunk;
        return o > sz - kBsgChunk ? sz - kBsgChunk : o;
    };
    auto stripe_of = [&](uint32_t vs) { return TBL ? vs % ns : vs; };
    const bool builder = wave < static_cast<uint32_t>(P);
    // the input this wave transposes next, loaded one phase ahead (the next
    // unit's first phase while the current unit's last phase computes), so a
    // phase never starts waiting on HBM
    u32x4 xin[4];
    auto load_input = [&](uint32_t vs, uint32_t cu, uint32_t j) {
        const uint8_t* ip = src.in(j) + (stripe_of(vs) * job.in_sstride + unit_off(cu) + lane * 16u);
        xin[0] = load16(ip);
        xin[1] = load16(ip + 1024);
        xin[2] = load16(ip + 2048);
        xin[3] = load16(ip + 3072);
    };
    uint32_t s = blockIdx.x / job.cps, c = blockIdx.x - s * job.cps;  // s: (group, stripe) index
    if (builder && s < nvs && wave < k) load_input(s, c, wave);
    while (s < nvs) {
        uint32_t s2 = s + job.gs_s, c2 = c + job.gs_c;  // this workgroup's next unit
        if (c2 >= job.cps) {
            c2 -= job.cps;
            ++s2;
        }
        const uint32_t g = TBL ? s / ns : 0u;  // row group
        const uint32_t row0 = g * rpg, rows = r - row0 < rpg ? r - row0 : rpg;
        const KWords cw = src.coef() + (g * 4u + wave) * nph * ND;  // this wave's phases
        const uint64_t ob = stripe_of(s) * job.out_sstride + unit_off(c) + lane * 16u;
        uint32_t acc[RT][2][8];
#pragma unroll
        for (int rr = 0; rr < RT; ++rr)
#pragma unroll
            for (int gg = 0; gg < 2; ++gg)
#pragma unroll
                for (int b = 0; b < 8; ++b) acc[rr][gg][b] = 0u;
        for (uint32_t f = 0; f < nph; ++f) {
            const uint32_t j0 = f * P;
            // build: input j0 + wave into slot wave
            const uint32_t jb = j0 + wave;
            if (builder && jb < k) {
                char* slot = bsg_lds + wave * kBsgSlotBytes;
                uint32_t g0[8] = {xin[0].x, xin[0].y, xin[0].z, xin[0].w, xin[1].x, xin[1].y, xin[1].z, xin[1].w};
                uint32_t g1[8] = {xin[2].x, xin[2].y, xin[2].z, xin[2].w, xin[3].x, xin[3].y, xin[3].z, xin[3].w};
                transpose8(g0);
                transpose8(g1);
                const uint32_t l0[4] = {g0[0], g0[1], g0[2], g0[3]}, l1[4] = {g1[0], g1[1], g1[2], g1[3]};
                const uint32_t h0[4] = {g0[4], g0[5], g0[6], g0[7]}, h1[4] = {g1[4], g1[5], g1[6], g1[7]};
                write_combos(slot, lane8, l0, l1, 0u);
                write_combos(slot, lane8, h0, h1, 16u);
            }
            if (builder) {  // prefetch: this unit's next phase, else the next unit's first
                if (f + 1 < nph) {
                    if (jb + P < k) load_input(s, c, jb + P);
                } else if (s2 < nvs && wave < k) {
                    load_input(s2, c2, wave);
                }
            }
            // this phase's coefficients (scalar loads, waited for before the barrier)
            uint32_t cwd[ND];
#pragma unroll
            for (int d = 0; d < ND; ++d) cwd[d] = cw[f * ND + d];
            auto coef_at = [&](int t) { return (cwd[t >> 2] >> ((t & 3) * 8)) & 0xFFu; };
            __syncthreads();
            const uint32_t jn = k - j0 < static_cast<uint32_t>(P) ? k - j0 : static_cast<uint32_t>(P);
            uint32_t o[16];
#pragma unroll
            for (int b = 0; b < 16; ++b) o[b] = g_bsg.off[coef_at(0) * 16u + b];
#pragma unroll
            for (int t = 0; t < P * RT; ++t) {
                const int js = t / RT, rr = t % RT;
                if (static_cast<uint32_t>(js) >= jn) break;  // wave-uniform
                uint32_t on[16];
                if (t + 1 < P * RT) {  // the next step's offsets, in flight during this step
#pragma unroll
                    for (int b = 0; b < 16; ++b) on[b] = g_bsg.off[coef_at(t + 1) * 16u + b];
                }
                const char* base = bsg_lds + js * kBsgSlotBytes + lane8;
#pragma unroll
                for (int b = 0; b < 8; ++b) {
                    const u32x2 vl = *reinterpret_cast<const u32x2*>(base + o[b]);
                    const u32x2 vh = *reinterpret_cast<const u32x2*>(base + o[8 + b]);
                    acc[rr][0][b] = xor3(acc[rr][0][b], vl.x, vh.x);
                    acc[rr][1][b] = xor3(acc[rr][1][b], vl.y, vh.y);
                }
                if (t + 1 < P * RT) {
#pragma unroll
                    for (int b = 0; b < 16; ++b) o[b] = on[b];
                }
            }
            __syncthreads();  // every wave has read the slots before the next phase overwrites them
        }
#pragma unroll
        for (int rr = 0; rr < RT; ++rr) {
            const uint32_t i = wave + 4u * rr;
            if (i >= rows) break;  // wave-uniform
            transpose8(acc[rr][0]);
            transpose8(acc[rr][1]);
            uint8_t* op = src.out(row0 + i) + ob;
            store16_out<true>(op, u32x4{acc[rr][0][0], acc[rr][0][1], acc[rr][0][2], acc[rr][0][3]});
            store16_out<true>(op + 1024, u32x4{acc[rr][0][4], acc[rr][0][5], acc[rr][0][6], acc[rr][0][7]});
            store16_out<true>(op + 2048, u32x4{acc[rr][1][0], acc[rr][1][1], acc[rr][1][2], acc[rr][1][3]});
            store16_out<true>(op + 3072, u32x4{acc[rr][1][4], acc[rr][1][5], acc[rr][1][6], acc[rr][1][7]});
        }
        s = s2;
        c = c2;
    }
}

// ---------------------------------------------------------------------------
// matapply_bsr<RT>: bit-sliced with the coefficients as run-time data, at the
// instruction count of a specialised (JIT) kernel.  Multiplying the 32 bytes
// of a lane by c and adding them to an accumulator row is, on bit-planes, eight
// XOR3s whose operands depend on c only; gf_routines.inc holds those eight
// instructions for every c as a routine (zfec_gf_routines + 72 c) working on
// fixed registers: the input's combinations of planes (built once per input
// per wave) and accumulator row 0, offset to row rr by VGPR index mode.  A
// coefficient costs a call (a few scalar instructions and two jumps, no LDS
// read) instead of matapply_bsg's sixteen LDS reads or a compile per matrix.
//
// Unit = 2 KiB of every block of a stripe (32 bytes per lane, like the JIT
// kernels); rows in tiles of <= RT <= 10 (the accumulators of a tile live in
// v38..v37+8RT, gf_routines.inc).  Two forms:
//   matapply_bsr_solo<RT> (one tile, r <= 10): one wave per unit, no LDS; the
//       wave loads and transposes its inputs two ahead;
//   matapply_bsr<RT> ("lds", r > 10): one workgroup per unit, a wave per
//       tile; the unit's inputs go through LDS in phases, loaded straight into
//       LDS (LDS-DMA) and transposed in place into bit-planes, two phases
//       resident so the next phase loads while the waves walk the current one
//       (bsr_db_phase).  All k inputs in LDS at once (k * 2 KiB) capped the
//       workgroups per CU and measured 0.51 ms against 0.37-0.38 with phases
//       of 8 on cfg4's first-seen decodes (profiles/r04_bsr_ab.json).
// Coefficients: absolute routine addresses (BsrJob / BsrTblJob below).
// ---------------------------------------------------------------------------
// ZFEC_GF_ROUTINES_INC: another generated form of the routines (the A/B,
// tools/ab_bsr.sh: `tools/gen_gf_routines.py --form legacy --out ...`)
#ifdef ZFEC_GF_ROUTINES_INC
#include ZFEC_GF_ROUTINES_INC
#else
#include "gf_routines.inc"
#endif

constexpr uint32_t kBsrChunk = 2048;  // bytes of each block per unit
template <bool B>
struct BoolC {  // a compile-time flag passed to generic lambdas
    static constexpr bool value = B;
};
typedef __attribute__((address_space(1))) void GlobalVoid;
typedef __attribute__((address_space(3))) void LdsVoid;
// Inputs per phase of the combination-sharing form (7.5 KiB of combinations +
// 2 KiB of raw staging each): one per wave, so the 16 / nw workgroups a CU
// holds at 4 waves per SIMD take 152 KiB.
__host__ __device__ constexpr uint32_t bsr_cmb_phase(uint32_t nw) { return nw; }
// Inputs per phase of the plane-sharing form, whose LDS holds two phases: the
// 16 / nw workgroups a CU holds at 4 waves per SIMD keep within its 160 KiB.
__host__ __device__ constexpr uint32_t bsr_db_phase(uint32_t nw) { return nw <= 2 ? 2u : nw <= 4 ? 4u : 8u; }
constexpr int kBsrMaxOut = 4 * kBsrMaxRows;  // rows of the kernel-argument form (4 tiles)
constexpr int kBsrArgAddrs = 432;     // routine addresses the kernel-argument form holds

// Routine addresses: every coefficient reaches the kernel as the absolute
// address of its routine (zfec_gf_routines + 72 c on the launch's device,
// bsr_routine_base), in the kernel's walk order [group][wave][input][row],
// RT per (wave, input) -- rows past a wave's tile hold routine 0's address,
// which only returns.  Kernel-argument form (k <= 32, r <= 40, at most
// kBsrArgAddrs addresses): block pointers and addresses in the arguments.
struct alignas(16) BsrJob {
    uint64_t sz, in_sstride, out_sstride;
    uint32_t nstripes, k, r, cps, gs_c, gs_s;
    uint32_t nt;  // one-wave form: row tiles per unit
    uint32_t pad_;
    const uint8_t* in[kMaxIn];
    uint8_t* out[kBsrMaxOut];
    uint64_t addr[kBsrArgAddrs];
};
static_assert(sizeof(BsrJob) <= 4096, "kernel arguments are limited to 4 KiB");

// Table form (k > 32, or more addresses than the arguments hold): the block
// pointers in the arguments, the addresses in a device-side table the host
// uploads once per matrix and layout and keeps (bsr_addr_table), read with
// scalar loads.
constexpr int kBsrTblPtrs = 320;  // k + r block pointers of a table-form launch
struct alignas(16) BsrTblJob {
    uint64_t sz, in_sstride, out_sstride;
    uint32_t nstripes, k, r, cps, gs_c, gs_s;
    uint32_t ngroups;  // row groups: workgroup units are (group, stripe, unit) triples
    uint32_t pad_;
    const uint64_t* addr;             // device: [group][wave][input][RT] routine addresses
    const uint8_t* ptr[kBsrTblPtrs];  // k input block pointers, then r output block pointers
};
static_assert(sizeof(BsrTblJob) <= 4096, "kernel arguments are limited to 4 KiB");

// Mix form (a pattern per stripe; 4 < k <= 32, r <= kRepairMaxRows): every
// pattern's r x k matrix is a record in device memory -- its routine addresses
// in the walk order [wave][input][RT] (fill_bsr_addrs with one group, no input
// split), then one dword live-row mask (bit i: row i is stored), padded to 16
// bytes -- and ids[s] names the record of stripe s.  The tiles depend on r
// alone (bsr_mix_tiles), so a record built once serves every call.  Ids,
// records and masks are only read, by scalar loads: an earlier copy or kernel
// of the stream wrote them (the scalar cache starts every kernel empty).
constexpr int kBsrMixPtrs = kMaxIn + static_cast<int>(kRepairMaxRows);
struct alignas(16) BsrMixJob {
    uint64_t sz, in_sstride, out_sstride;
    uint32_t nstripes, k, r, cps, gs_c, gs_s;
    uint32_t npatterns;
    uint32_t stride;                  // uint64 words per record
    const uint32_t* ids;              // device: nstripes pattern ids
    const uint64_t* records;          // device: npatterns records
    const uint8_t* ptr[kBsrMixPtrs];  // k input block pointers, then r output block pointers
};
static_assert(sizeof(BsrMixJob) <= 4096, "kernel arguments are limited to 4 KiB");

// Reads input j's RT routine addresses (scalar loads).
// (The row offset is added to a 64-bit pointer, so the loads share one
// address and merge into s_load_dwordx16 / x4 with immediate offsets.)
template <int RT>
__device__ __forceinline__ void bsr_addrs(uint64_t (&ad)[RT], CU64 ca, uint32_t j) {
    const CU64 q = ca + static_cast<uint64_t>(j) * RT;
#pragma unroll
    for (int rr = 0; rr < RT; ++rr) ad[rr] = q[rr];
}

// The address of zfec_gf_routines on this device, computed the way a call
// site would (s_getpc + the rel32 relocation) and stored by lane 0 with a
// vector store; the host reads it once per device (bsr_routine_base).
__global__ void bsr_table_probe(uint64_t* out) {
    uint32_t lo, hi;
    asm volatile(
        "s_getpc_b64 s[26:27]\n\t"
        "s_add_u32 s26, s26, zfec_gf_routines@rel32@lo+4\n\t"
        "s_addc_u32 s27, s27, zfec_gf_routines@rel32@hi+12\n\t"
        "s_mov_b32 %0, s26\n\t"
        "s_mov_b32 %1, s27"
        : "=s"(lo), "=s"(hi)
        :
        : "s26", "s27", "scc");
    if (threadIdx.x == 0) out[0] = (static_cast<uint64_t>(hi) << 32) | lo;
}

// The 30 combinations of an input's bit-planes in bsr_input_c's register
// order (gf_routines.inc): planes p0..p7, then L[m] (planes 0-3) and H[m]
// (planes 4-7) for the eleven multi-plane m in increasing order.
__device__ __forceinline__ void bsr_combos(const uint32_t (&p)[8], uint32_t (&q)[30]) {
    constexpr int kMulti[11] = {3, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15};
#pragma unroll
    for (int i = 0; i < 8; ++i) q[i] = p[i];
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        uint32_t c[16] = {};
#pragma unroll
        for (int i = 0; i < 4; ++i) c[1 << i] = p[4 * side + i];
#pragma unroll
        for (int x = 0; x < 11; ++x) {
            const int m = kMulti[x];
            const int top = m >= 8 ? 8 : m >= 4 ? 4 : 2;
            c[m] = c[m ^ top] ^ c[top];
            q[8 + 11 * side + x] = c[m];
        }
    }
}

// Bytes of LDS per input of a phase: the 8 planes, or (CMB) all 30 combinations.
template <bool CMB>
__host__ __device__ constexpr uint32_t bsr_in_bytes() {
    return CMB ? 30u * 256u : 8u * 256u;
}

// Verify forms (matverify_bsr, fec_verify_batch): the argument blocks of
// BsrJob / BsrTblJob with the stored check rows where the outputs were (they
// share the inputs' stripe stride, so out_sstride's place holds the mismatch
// words) and the words' geometry.  k <= 32 and r <= 40 only: 72 block pointers
// in the table form.
struct alignas(16) BsrVfyJob {
    uint64_t sz, in_sstride;
    uint32_t* mismatch;
    uint32_t nstripes, k, r, cps, gs_c, gs_s;
    uint32_t words, bit0;  // mismatch words per stripe; bit index of row 0
    const uint8_t* in[kMaxIn];
    const uint8_t* out[kBsrMaxOut];  // the stored check rows
    uint64_t addr[kBsrArgAddrs];
};
static_assert(sizeof(BsrVfyJob) <= 4096, "kernel arguments are limited to 4 KiB");

constexpr int kBsrVfyPtrs = kMaxIn + kBsrMaxOut;
struct alignas(16) BsrVfyTblJob {
    uint64_t sz, in_sstride;
    uint32_t* mismatch;
    uint32_t nstripes, k, r, cps, gs_c, gs_s;
    uint32_t ngroups;  // 1
    uint32_t words, bit0;
    uint32_t pad_;
    const uint64_t* addr;             // device: [wave][input][RT] routine addresses
    const uint8_t* ptr[kBsrVfyPtrs];  // k input block pointers, then r stored check rows
};
static_assert(sizeof(BsrVfyTblJob) <= 4096, "kernel arguments are limited to 4 KiB");

// f(integral_constant<int, I>) for I = I0 .. N - 1: a loop whose index is a
// compile-time value.
template <int I, int N, class F>
__device__ __forceinline__ void bsr_static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        bsr_static_for<I + 1, N>(f);
    }
}

// A stored row's two pieces into the plane and combination registers the walk
// has left dead (v8..v31, eight per prefetch slot), at the point of use: left
// to itself the allocator put them in v0..v7 and spilled the unit loop's
// invariants around the epilogue at RT = 10.
template <int S>
__device__ __forceinline__ void bsr_verify_pin(u32x4& a, u32x4& b) {
    static_assert(S >= 0 && S < 3, "three prefetch slots");
    if constexpr (S == 0)
        asm volatile("" : "+{v[8:11]}"(a), "+{v[12:15]}"(b));
    else if constexpr (S == 1)
        asm volatile("" : "+{v[16:19]}"(a), "+{v[20:23]}"(b));
    else
        asm volatile("" : "+{v[24:27]}"(a), "+{v[28:31]}"(b));
}

// The verify epilogue of a wave's tile: the computed rows stay bit-planes in
// acc; each live row's stored 32 bytes per lane (at chk(rr) + ib and + 1024)
// are transposed into planes, XOR-ed in and OR-ed into one dword -- the
// syndrome is nonzero iff some plane is, so acc is never transposed back --
// and one ballot per row builds the wave-uniform mask that one lane ORs into
// the stripe's words (mismatch_or; clean data: no store, no atomic).  Stored
// rows are loaded two rows ahead of their use for RT <= 9 (rows rr + 1 and
// rr + 2 in flight while row rr is compared: three slots of 8 VGPRs), one row
// ahead at RT = 10; the loads are unconditional, past the tile's last row
// they re-read it, so no load sits under a branch.
template <int RT, class C>
__device__ __forceinline__ void bsr_verify_rows(uint32_t (&acc)[RT][8], uint32_t rows, uint64_t ib, C chk,
                                                uint32_t* words, uint32_t bit) {
    if (rows == 0u) return;  // (wave-uniform; bsr_tiles never leaves a wave without rows)
    // rows resident: the one compared and D - 1 in flight (one at RT = 10, where
    // 80 accumulator registers leave the LDS form's 128 no room for the third)
    constexpr int D = RT < 3 ? RT : RT < 10 ? 3 : 2;
    // RT = 10: the next row's loads are issued after the current row's
    // transpose (whose temporaries are dead by then), not before it, and the
    // rows run straight-line -- a row past the tile is compared too, its
    // result dropped -- so that the loads stay out of branches
    constexpr bool LATE = RT >= 10;
    u32x4 y0[D], y1[D];
    auto fetch = [&](int slot, uint32_t rr) {
        const uint8_t* p = chk(rr < rows ? rr : rows - 1u) + ib;
        y0[slot] = load16(p);
        y1[slot] = load16(p + 1024);
    };
#pragma unroll
    for (int rr = 0; rr < D - 1; ++rr) fetch(rr, rr);
    uint32_t mask = 0;
    // (rows by compile-time index: the slot's registers are named in bsr_verify_pin)
    bsr_static_for<0, RT>([&](auto rc) {
        constexpr int rr = decltype(rc)::value, slot = rr % D, ahead = rr + D - 1;
        if constexpr (LATE) {
            u32x4 a = y0[slot], b = y1[slot];
            bsr_verify_pin<slot>(a, b);
            uint32_t v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            transpose8(v);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (ahead < RT) fetch(ahead % D, ahead);
            uint32_t d = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) d |= acc[rr][i] ^ v[i];
            if (static_cast<uint32_t>(rr) < rows && __builtin_amdgcn_ballot_w64(d != 0u) != 0ull) mask |= 1u << rr;
        } else {
            if constexpr (ahead < RT) fetch(ahead % D, ahead);
            if (static_cast<uint32_t>(rr) < rows) {  // wave-uniform
                u32x4 a = y0[slot], b = y1[slot];
                bsr_verify_pin<slot>(a, b);
                uint32_t v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
                transpose8(v);
                uint32_t d = 0;
#pragma unroll
                for (int i = 0; i < 8; ++i) d |= acc[rr][i] ^ v[i];
                if (__builtin_amdgcn_ballot_w64(d != 0u) != 0ull) mask |= 1u << rr;
            }
        }
    });
    if (mask != 0u) {  // wave-uniform; the rare path
        // the lane number and the mask enter vector registers here: formed as
        // loop invariants (the lane-0 flag, mismatch_or's 64-bit constants for
        // a scalar mask) they were held across the walk and spilled at RT = 10
        uint32_t l = 0u, m = mask;
        asm volatile("" : "+v"(l), "+v"(m));
        l = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, l));  // the lane, formed here
        if (l == 0u) mismatch_or(words, bit, m);
    }
}

// The LDS-phase kernel.  Its verify form is this kernel instantiated on a
// verify job (J = BsrVfyJob: matverify_bsr<RT,lds>; BsrVfyTblJob:
// matverify_bsr<RT,lds,tbl>; CMB = false -- 2 or 4 waves for k <= 32): the
// same walk, the epilogue comparing the rows with the stored check rows
// instead of storing them (no store to block memory).  The mode hangs on the
// job type so that the apply instantiations keep their symbols and their code.
template <int RT, bool TBL, bool CMB, class J>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4))) void matapply_bsr(const J job) {
    constexpr bool VFY = std::is_same<J, BsrVfyJob>::value || std::is_same<J, BsrVfyTblJob>::value;
    static_assert(!VFY || !CMB, "the verify forms share planes, not combinations");
    // J = BsrMixJob (matapply_bsr<RT,lds,mix>): a pattern id per stripe picks the
    // record the routine addresses and the live-row mask are read from
    constexpr bool MIX = std::is_same<J, BsrMixJob>::value;
    static_assert(!MIX || (TBL && !CMB), "the mix form: block pointers as the table form's, planes shared");
    // [input][half][lane] planes, or (CMB) [input][7 x (4 dwords)][lane] + [2 dwords][lane] combinations
    extern __shared__ u32x4 bsr_planes[];
    constexpr uint32_t kIn = bsr_in_bytes<CMB>() / 16;  // u32x4 per input
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t nw = blockDim.x >> 6;
    const uint32_t k = job.k, r = job.r;
    // block pointers and routine addresses: kernel arguments (BsrJob) or the
    // device-side table (BsrTblJob); the walk's "stripes" are (row group,
    // stripe) pairs, group-major
    const uint32_t ns = job.nstripes;
    uint32_t ng = 1;
    KPtr<J> kj = kernarg_job<J>();
    if constexpr (TBL && !MIX) ng = job.ngroups;
    auto in_ptr = [&](uint32_t j) -> const uint8_t* {
        if constexpr (TBL)
            return kj->ptr[j];
        else
            return kj->in[j];
    };
    auto out_ptr = [&](uint32_t i) -> uint8_t* {
        if constexpr (TBL)
            return const_cast<uint8_t*>(kj->ptr[k + i]);
        else
            return const_cast<uint8_t*>(kj->out[i]);  // (VFY: the stored check rows, only read)
    };
    const uint64_t sz = job.sz;
    uint32_t s = blockIdx.x / job.cps, c = blockIdx.x - s * job.cps;
    auto advance = [&] {  // the grid-stride step, with its carry
        c += job.gs_c;
        s += job.gs_s;
        if (c >= job.cps) {
            c -= job.cps;
            ++s;
        }
    };
    while (s < ns * ng) {
        const uint32_t g = TBL && ng > 1 ? s / ns : 0u, stripe = s - g * ns;
        const uint32_t gr0 = g * r / ng, grn = (g + 1) * r / ng - gr0;
        const uint32_t r0 = gr0 + wave * grn / nw, rows = gr0 + (wave + 1) * grn / nw - r0;
        uint32_t id = 0;
        if constexpr (MIX) {
            // the stripe's id: one scalar load, the same in every wave of the
            // workgroup; an id that names no record skips the unit before any
            // record read and any barrier, and nothing of the stripe is written
            // (the id's fields by a fresh look at the arguments, not held across the walk)
            const KPtr<J> km = kernarg_job<J>();
            id = __builtin_amdgcn_readfirstlane(((CU32)km->ids)[stripe]);
            if (id >= km->npatterns) {
                advance();
                continue;
            }
        }
        const CU64 ca = [&] {
            if constexpr (MIX) {
                const KPtr<J> km = kernarg_job<J>();
                return (CU64)km->records + static_cast<uint64_t>(id) * km->stride + wave * k * RT;
            } else if constexpr (TBL)
                return (CU64)job.addr + (g * nw + wave) * k * RT;
            else
                return (CU64)kj->addr + wave * k * RT;
        }();
        uint64_t off = static_cast<uint64_t>(c) * kBsrChunk;
        if (off > sz - kBsrChunk) off = sz - kBsrChunk;  // the last unit ends at sz (overlapping its neighbour)
        const uint64_t ib = stripe * job.in_sstride + off + lane * 16u;
        uint64_t ob = 0;
        if constexpr (!VFY) ob = stripe * job.out_sstride + off + lane * 16u;
        uint32_t acc[RT][8];  // no zeroing: the wave's first input calls "set" routines (kBsrSetBase)
        // One input's calls: its planes (or, CMB, its 30 combinations) read from
        // LDS at b, its routine addresses in `cur`; the wave's first input
        // (global index 0) calls the set twins (bsr_input_first: every row
        // written).  `wait` runs between the LDS reads and the calls.
        constexpr int kVals = CMB ? 30 : 8;
        auto load = [&](const u32x4* b, uint32_t (&q)[kVals]) {
            if constexpr (CMB) {
#pragma unroll
                for (int g = 0; g < 7; ++g) {
                    const u32x4 t = b[g * 64 + lane];
                    q[4 * g] = t.x;
                    q[4 * g + 1] = t.y;
                    q[4 * g + 2] = t.z;
                    q[4 * g + 3] = t.w;
                }
                const u32x2 t2 = reinterpret_cast<const u32x2*>(b + 448)[lane];
                q[28] = t2.x;
                q[29] = t2.y;
            } else {
                const u32x4 pa = b[lane], pb = b[64u + lane];
                q[0] = pa.x, q[1] = pa.y, q[2] = pa.z, q[3] = pa.w;
                q[4] = pb.x, q[5] = pb.y, q[6] = pb.z, q[7] = pb.w;
            }
        };
        auto input = [&](auto first, const uint32_t (&q)[kVals], const uint64_t (&cur)[RT]) {
            if constexpr (CMB) {
                if constexpr (decltype(first)::value)
                    bsr_input_c_first<RT>(acc, q, cur);
                else
                    bsr_input_c<RT>(acc, q, cur);
            } else {
                if constexpr (decltype(first)::value)
                    bsr_input_first<RT>(acc, q, cur);
                else
                    bsr_input<RT>(acc, q, cur);
            }
        };
        // calls(first, ph, kn, o): the calls of one phase's kn inputs (ph, ph +
        // 1, ...), planes or combinations at LDS offset o (u32x4).  The first
        // phase is its own instance (first = BoolC<true>): its input 0 runs the
        // set twins, peeled at compile time -- a run-time choice between the two
        // statements made the compiler copy and spill the pinned accumulators.
        //
        // Routine addresses, two sets by the parity of the input's global
        // index (phases hold an even number of inputs: bsr_db_phase,
        // bsr_cmb_phase).  Input g + 1's set is loaded (scalar loads) right
        // after input g's LDS data has been waited for and before g's calls,
        // so it arrives during them: the wait for g + 1's LDS data, which
        // drains scalar loads too (lgkmcnt), finds it landed.  Round 5 loaded
        // input g + 2's set after g's calls, and that wait stalled on it.
        uint64_t ad0[RT], ad1[RT];
        bsr_addrs<RT>(ad0, ca, 0);
        auto step = [&](auto first, uint32_t gi, const u32x4* b, const uint64_t (&cur)[RT], uint64_t (&nxt)[RT]) {
            uint32_t q[kVals];
            load(b, q);
            // a use of every value read: the LDS wait goes here, before the scalar loads
            if constexpr (CMB)
                asm volatile("" ::"v"(q[3]), "v"(q[7]), "v"(q[11]), "v"(q[15]), "v"(q[19]), "v"(q[23]), "v"(q[27]),
                             "v"(q[29]));
            else
                asm volatile("" ::"v"(q[3]), "v"(q[7]));
            __builtin_amdgcn_sched_barrier(0);
            bsr_addrs<RT>(nxt, ca, gi + 1 < k ? gi + 1 : k - 1);  // unconditional (clamped)
            __builtin_amdgcn_sched_barrier(0);
            input(first, q, cur);
        };
        auto calls = [&](auto first, uint32_t ph, uint32_t kn, uint32_t o) {
            uint32_t j = 0;
            if constexpr (decltype(first)::value) {  // ph == 0
                step(BoolC<true>{}, 0, bsr_planes + o, ad0, ad1);
                for (j = 1; j + 1 < kn; j += 2) {
                    step(BoolC<false>{}, j, bsr_planes + o + j * kIn, ad1, ad0);
                    step(BoolC<false>{}, j + 1, bsr_planes + o + (j + 1) * kIn, ad0, ad1);
                }
                if (j < kn) step(BoolC<false>{}, j, bsr_planes + o + j * kIn, ad1, ad0);  // k < the phase
                return;
            }
            for (; j + 1 < kn; j += 2) {
                step(first, ph + j, bsr_planes + o + j * kIn, ad0, ad1);
                step(first, ph + j + 1, bsr_planes + o + (j + 1) * kIn, ad1, ad0);
            }
            if (j < kn) step(first, ph + j, bsr_planes + o + j * kIn, ad0, ad1);  // the last phase
        };
        if constexpr (!CMB) {
            // Planes: double-buffered phases of kq inputs.  A phase's inputs go
            // straight into LDS (LDS-DMA, global_load_lds: no registers in
            // flight) while the waves run the previous phase's calls, and are
            // then transposed in place -- lane l's 16 + 16 bytes land in the
            // slots its planes go to (b[l], b[64 + l]).  One barrier per phase.
            const uint32_t kq = bsr_db_phase(nw);
            auto dma = [&](uint32_t ph, uint32_t kn, uint32_t o) {
                for (uint32_t j = wave; j < kn; j += nw) {
                    const uint8_t* ip = in_ptr(ph + j) + ib;
                    u32x4* b = bsr_planes + o + j * kIn;
                    __builtin_amdgcn_global_load_lds((const GlobalVoid*)(ip), (LdsVoid*)(b), 16, 0, 0);
                    __builtin_amdgcn_global_load_lds((const GlobalVoid*)(ip + 1024), (LdsVoid*)(b + 64), 16, 0, 0);
                }
            };
            auto xpose = [&](uint32_t kn, uint32_t o) {
                // hipcc does not order these LDS reads after the LDS-DMA writes
                // (no vmcnt wait of its own here): wait for them explicitly
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                for (uint32_t j = wave; j < kn; j += nw) {
                    u32x4* b = bsr_planes + o + j * kIn;
                    const u32x4 x0 = b[lane], x1 = b[64u + lane];
                    uint32_t v[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
                    transpose8(v);
                    b[lane] = u32x4{v[0], v[1], v[2], v[3]};
                    b[64u + lane] = u32x4{v[4], v[5], v[6], v[7]};
                }
            };
            uint32_t kn = k < kq ? k : kq, o = 0;
            dma(0, kn, 0);
            xpose(kn, 0);
            __syncthreads();
            auto phase = [&](auto first, uint32_t ph) {
                const uint32_t nx = ph + kq, knx = nx < k ? (k - nx < kq ? k - nx : kq) : 0u;
                const uint32_t ox = o ^ (kq * kIn);  // the other half
                if (knx) dma(nx, knx, ox);
                calls(first, ph, kn, o);
                if (knx) xpose(knx, ox);
                __syncthreads();  // phase ph's planes read, phase nx's written
                kn = knx;
                o = ox;
            };
            phase(BoolC<true>{}, 0);
            for (uint32_t ph = kq; ph < k; ph += kq) phase(BoolC<false>{}, ph);
        } else {
            // Combinations: phases of kp = nw inputs, one per wave.  A phase's
            // inputs go into a raw staging area (LDS-DMA) while the waves walk
            // the previous phase; after the barrier that ends it, each wave
            // transposes its own input, builds its 30 combinations and writes
            // them for every wave.
            const uint32_t kp = bsr_cmb_phase(nw), oraw = (k < kp ? k : kp) * kIn;  // staging after the combinations
            auto dma = [&](uint32_t ph, uint32_t kn) {
                for (uint32_t j = wave; j < kn; j += nw) {
                    const uint8_t* ip = in_ptr(ph + j) + ib;
                    u32x4* b = bsr_planes + oraw + j * 128u;
                    __builtin_amdgcn_global_load_lds((const GlobalVoid*)(ip), (LdsVoid*)(b), 16, 0, 0);
                    __builtin_amdgcn_global_load_lds((const GlobalVoid*)(ip + 1024), (LdsVoid*)(b + 64), 16, 0, 0);
                }
            };
            auto build = [&](uint32_t kn) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (as in the planes form)
                for (uint32_t j = wave; j < kn; j += nw) {
                    const u32x4* r = bsr_planes + oraw + j * 128u;
                    const u32x4 x0 = r[lane], x1 = r[64u + lane];
                    uint32_t v[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
                    transpose8(v);
                    uint32_t q30[30];
                    bsr_combos(v, q30);
                    u32x4* b = bsr_planes + j * kIn;
#pragma unroll
                    for (int g = 0; g < 7; ++g)
                        b[g * 64 + lane] = u32x4{q30[4 * g], q30[4 * g + 1], q30[4 * g + 2], q30[4 * g + 3]};
                    reinterpret_cast<u32x2*>(b + 448)[lane] = u32x2{q30[28], q30[29]};
                }
            };
            uint32_t kn = k < kp ? k : kp;
            dma(0, kn);
            build(kn);
            __syncthreads();
            auto phase = [&](auto first, uint32_t ph) {
                const uint32_t nx = ph + kp, knx = nx < k ? (k - nx < kp ? k - nx : kp) : 0u;
                if (knx) dma(nx, knx);  // each wave's staging slot: read by its own build() before the barrier
                calls(first, ph, kn, 0);
                __syncthreads();  // every wave has read the combinations before they are overwritten
                if (knx) {
                    build(knx);
                    __syncthreads();
                }
                kn = knx;
            };
            phase(BoolC<true>{}, 0);
            for (uint32_t ph = kp; ph < k; ph += kp) phase(BoolC<false>{}, ph);
        }
        if constexpr (VFY) {
            (void)ob;
            // the words' geometry is read here, after the walk (a fresh look at
            // the arguments): held across it, it spilled at RT = 10
            const KPtr<J> kv = kernarg_job<J>();
            uint64_t so = stripe * kv->in_sstride + off;  // ib again, not held in vector registers meanwhile
            asm volatile("" : "+s"(so));
            bsr_verify_rows<RT>(acc, rows, so + lane * 16u, [&](uint32_t rr) { return out_ptr(r0 + rr); },
                                kv->mismatch + static_cast<uint64_t>(stripe) * kv->words, kv->bit0 + r0);
        } else {
            // MIX: the record's live-row mask (the dword after its nw tiles of
            // addresses), read here, after the walk; a row whose bit is clear
            // is not stored
            uint32_t live = ~0u;
            if constexpr (MIX)
                live = __builtin_amdgcn_readfirstlane(((CU32)(ca + (nw - wave) * k * RT))[0]) >> r0;
#pragma unroll
            for (int rr = 0; rr < RT; ++rr) {
                if (static_cast<uint32_t>(rr) < rows && ((live >> rr) & 1u)) {  // wave-uniform
                    transpose8(acc[rr]);
                    uint8_t* op = out_ptr(r0 + rr) + ob;
                    store16_out<true>(op, u32x4{acc[rr][0], acc[rr][1], acc[rr][2], acc[rr][3]});
                    store16_out<true>(op + 1024, u32x4{acc[rr][4], acc[rr][5], acc[rr][6], acc[rr][7]});
                }
            }
        }
        advance();
    }
}

// One wave's walk over n inputs of a unit (the one-wave and ks forms): input
// j's two 16-byte pieces at ptr(j) + ib, its routine addresses at ca[j * RT].
// Unrolled by two with fixed register roles (A: even inputs, B: odd), so a
// load lands in the registers its input's transpose has just consumed (no
// copies) and is waited for two inputs later; the A and B routine-address
// sets are scalar-loaded the same way, and block pointers one step ahead of
// their use (a scalar wait drains every outstanding scalar load, so none is
// issued right before it is needed).
template <int RT, class P>
__device__ __forceinline__ void bsr_walk(uint32_t (&acc)[RT][8], uint32_t n, uint64_t ib, CU64 ca, P ptr) {
    u32x4 a0, a1, b0, b1;
    const uint8_t* pa = ptr(0);
    const uint8_t* pb = ptr(n > 1 ? 1 : 0);
    a0 = load16(pa + ib);
    a1 = load16(pa + ib + 1024);
    b0 = load16(pb + ib);
    b1 = load16(pb + ib + 1024);
    pa = ptr(n > 2 ? 2 : n - 1);
    pb = ptr(n > 3 ? 3 : n - 1);
    uint64_t ada[RT], adb[RT];
    bsr_addrs<RT>(ada, ca, 0);
    bsr_addrs<RT>(adb, ca, n > 1 ? 1 : 0);
    // the loads and scalar loads are unconditional (past the last input they
    // re-read input n - 1, from L2): a conditional load would make the compiler
    // merge its registers with a copy that waits for every load in flight
    auto step = [&](auto first, u32x4& x0, u32x4& x1, const uint8_t*& pn, uint64_t (&ad)[RT], uint32_t j) {
        uint32_t p[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
        transpose8(p);
        if constexpr (decltype(first)::value)  // the walk's first input: the set twins (fill_bsr_addrs)
            bsr_input_first<RT>(acc, p, ad);
        else
            bsr_input<RT>(acc, p, ad);
        // input j + 2 into x0 / x1 / ad, which this input has consumed (after
        // the calls, so the compiler cannot keep the planes in them and copy)
        bsr_addrs<RT>(ad, ca, j + 2 < n ? j + 2 : n - 1);
        x0 = load16(pn + ib);
        x1 = load16(pn + ib + 1024);
        pn = ptr(j + 4 < n ? j + 4 : n - 1);
    };
    // whole pairs, then an odd last input: with no conditional step inside the
    // loop, input j's wait leaves input j + 1's loads in flight.  Input 0 is
    // peeled (the set twins, a statement of its own: a run-time choice between
    // the two made the compiler copy the pinned accumulators).
    step(BoolC<true>{}, a0, a1, pa, ada, 0);
    uint32_t j = 1;
    for (; j + 1 < n; j += 2) {
        step(BoolC<false>{}, b0, b1, pb, adb, j);
        step(BoolC<false>{}, a0, a1, pa, ada, j + 1);
    }
    if (j < n) step(BoolC<false>{}, b0, b1, pb, adb, j);
}

// One wave per (unit, row tile), no LDS: the wave loads and transposes every
// input of its unit itself (tiles of one unit are adjacent workgroups, so the
// second tile's loads hit L2), two inputs in flight ahead.
template <int RT>
__global__ __launch_bounds__(64) void matapply_bsr_solo(const BsrJob job) {
    const uint32_t lane = threadIdx.x;
    const uint32_t k = job.k, r = job.r, nt = job.nt;
    const KPtr<BsrJob> kj = kernarg_job<BsrJob>();
    const uint64_t sz = job.sz;
    const uint64_t total = uint64_t(job.nstripes) * job.cps * nt;
    for (uint64_t v = blockIdx.x; v < total; v += gridDim.x) {
        const uint32_t t = static_cast<uint32_t>(v % nt);
        const uint64_t u = v / nt;
        const uint32_t s = static_cast<uint32_t>(u / job.cps), c = static_cast<uint32_t>(u % job.cps);
        const uint32_t r0 = t * r / nt, rows = (t + 1) * r / nt - r0;
        const CU64 ca = (CU64)kj->addr + t * k * RT;
        uint64_t off = static_cast<uint64_t>(c) * kBsrChunk;
        if (off > sz - kBsrChunk) off = sz - kBsrChunk;
        const uint64_t ib = s * job.in_sstride + off + lane * 16u;
        const uint64_t ob = s * job.out_sstride + off + lane * 16u;
        uint32_t acc[RT][8];  // no zeroing: the wave's first input calls "set" routines (kBsrSetBase)
        bsr_walk<RT>(acc, k, ib, ca, [&](uint32_t j) { return kj->in[j]; });
#pragma unroll
        for (int rr = 0; rr < RT; ++rr) {
            if (static_cast<uint32_t>(rr) < rows) {
                transpose8(acc[rr]);
                uint8_t* op = kj->out[r0 + rr] + ob;
                store16_out<true>(op, u32x4{acc[rr][0], acc[rr][1], acc[rr][2], acc[rr][3]});
                store16_out<true>(op + 1024, u32x4{acc[rr][4], acc[rr][5], acc[rr][6], acc[rr][7]});
            }
        }
    }
}

// The mix form of the one-wave kernel (matapply_bsr<RT,mix>; BsrMixJob, r <=
// 10): the unit's stripe, hence its pattern id and record, is the same in every
// lane -- read through readfirstlane and constant-address-space pointers, so id,
// addresses and mask are scalar loads.  An id that names no record skips the
// unit: nothing of the stripe is read or written.  The walk over units is the
// LDS-phase kernel's (c += gs_c, s += gs_s with the carry).
template <int RT>
__global__ __launch_bounds__(64) void matapply_bsr_mix_solo(const BsrMixJob job) {
    const uint32_t lane = threadIdx.x;
    const uint32_t k = job.k, r = job.r;
    const KPtr<BsrMixJob> kj = kernarg_job<BsrMixJob>();
    const uint64_t sz = job.sz;
    uint32_t s = blockIdx.x / job.cps, c = blockIdx.x - s * job.cps;
    auto advance = [&] {
        c += job.gs_c;
        s += job.gs_s;
        if (c >= job.cps) {
            c -= job.cps;
            ++s;
        }
    };
    while (s < job.nstripes) {
        // (the id's fields by a fresh look at the arguments, not held across the walk)
        const KPtr<BsrMixJob> km = kernarg_job<BsrMixJob>();
        const uint32_t id = __builtin_amdgcn_readfirstlane(((CU32)km->ids)[s]);
        if (id >= km->npatterns) {
            advance();
            continue;
        }
        const CU64 ca = (CU64)km->records + static_cast<uint64_t>(id) * km->stride;
        uint64_t off = static_cast<uint64_t>(c) * kBsrChunk;
        if (off > sz - kBsrChunk) off = sz - kBsrChunk;
        const uint64_t ib = s * job.in_sstride + off + lane * 16u;
        const uint64_t ob = s * job.out_sstride + off + lane * 16u;
        uint32_t acc[RT][8];  // no zeroing: the wave's first input calls "set" routines (kBsrSetBase)
        bsr_walk<RT>(acc, k, ib, ca, [&](uint32_t j) { return kj->ptr[j]; });
        const uint32_t live = __builtin_amdgcn_readfirstlane(((CU32)(ca + k * RT))[0]);  // the mask, after the walk
#pragma unroll
        for (int rr = 0; rr < RT; ++rr) {
            if (static_cast<uint32_t>(rr) < r && ((live >> rr) & 1u)) {  // wave-uniform
                transpose8(acc[rr]);
                uint8_t* op = const_cast<uint8_t*>(kj->ptr[k + rr]) + ob;
                store16_out<true>(op, u32x4{acc[rr][0], acc[rr][1], acc[rr][2], acc[rr][3]});
                store16_out<true>(op + 1024, u32x4{acc[rr][4], acc[rr][5], acc[rr][6], acc[rr][7]});
            }
        }
        advance();
    }
}

// matverify_bsr<RT>: the one-wave form's walk (one tile: r <= 10), then the
// verify epilogue instead of the stores.
template <int RT>
__global__ __launch_bounds__(64) void matverify_bsr_solo(const BsrVfyJob job) {
    const uint32_t lane = threadIdx.x;
    const uint32_t k = job.k, r = job.r;
    const KPtr<BsrVfyJob> kj = kernarg_job<BsrVfyJob>();
    const uint64_t sz = job.sz;
    const uint64_t total = uint64_t(job.nstripes) * job.cps;
    for (uint64_t u = blockIdx.x; u < total; u += gridDim.x) {
        const uint32_t s = static_cast<uint32_t>(u / job.cps), c = static_cast<uint32_t>(u % job.cps);
        uint64_t off = static_cast<uint64_t>(c) * kBsrChunk;
        if (off > sz - kBsrChunk) off = sz - kBsrChunk;
        const uint64_t ib = s * job.in_sstride + off + lane * 16u;
        uint32_t acc[RT][8];  // no zeroing: the wave's first input calls "set" routines (kBsrSetBase)
        bsr_walk<RT>(acc, k, ib, (CU64)kj->addr, [&](uint32_t j) { return kj->in[j]; });
        bsr_verify_rows<RT>(acc, r, ib, [&](uint32_t rr) { return kj->out[rr]; },
                            job.mismatch + static_cast<uint64_t>(s) * job.words, job.bit0);
    }
}

// Wide codes (k > 32) with one row tile (r <= 10), e.g. the reference
// benchmark's 94/100: a 64 MiB stripe is only a few hundred 2 KiB units, so
// the W waves of a workgroup split a unit's inputs (wave w: inputs
// [w k / W, (w + 1) k / W), loaded two ahead and transposed by the wave), XOR
// their partial accumulator planes into one LDS copy of the unit's rows
// (ds_xor_b32, [row][plane][lane]), and after a barrier wave w transposes and
// stores rows w, w + W, ...  Block pointers in the arguments, routine
// addresses ([group][input][RT]) in the device-side table (BsrTblJob).
template <int RT>
__global__ __launch_bounds__(512) void matapply_bsr_ks(const BsrTblJob job) {
    __shared__ uint32_t red[RT * 8 * 64];  // [row][plane][lane]
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t nw = blockDim.x >> 6;
    const uint32_t k = job.k, r = job.r;
    const KPtr<BsrTblJob> kj = kernarg_job<BsrTblJob>();
    const uint32_t j0 = wave * k / nw, j1 = (wave + 1) * k / nw;
    const uint32_t ns = job.nstripes, ng = job.ngroups;  // row groups of <= RT rows: (group, stripe) walk
    const uint64_t sz = job.sz;
    for (uint32_t i = threadIdx.x; i < RT * 8 * 64; i += blockDim.x) red[i] = 0u;
    __syncthreads();
    uint32_t s = blockIdx.x / job.cps, c = blockIdx.x - s * job.cps;
    while (s < ns * ng) {
        const uint32_t g = s / ns, stripe = s - g * ns;
        const uint32_t gr0 = g * r / ng, rows = (g + 1) * r / ng - gr0;
        const CU64 ca = (CU64)job.addr + g * k * RT;
        uint64_t off = static_cast<uint64_t>(c) * kBsrChunk;
        if (off > sz - kBsrChunk) off = sz - kBsrChunk;
        const uint64_t ib = stripe * job.in_sstride + off + lane * 16u;
        const uint64_t ob = stripe * job.out_sstride + off + lane * 16u;
        if (j0 < j1) {  // wave-uniform
            uint32_t acc[RT][8];  // no zeroing: input j0 calls "set" routines (kBsrSetBase)
            bsr_walk<RT>(acc, j1 - j0, ib, ca + j0 * RT,
                         [&](uint32_t j) { return kj->ptr[j0 + j]; });
#pragma unroll
            for (int rr = 0; rr < RT; ++rr)
                if (static_cast<uint32_t>(rr) < rows)
#pragma unroll
                    for (int b = 0; b < 8; ++b)
                        __hip_atomic_fetch_xor(&red[(rr * 8 + b) * 64 + lane], acc[rr][b], __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        __syncthreads();
        for (uint32_t i = wave; i < rows; i += nw) {  // wave-uniform
            uint32_t v[8];
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                v[b] = red[(i * 8 + b) * 64 + lane];
                red[(i * 8 + b) * 64 + lane] = 0u;  // ready for the next unit
            }
            transpose8(v);
            uint8_t* op = const_cast<uint8_t*>(kj->ptr[k + gr0 + i]) + ob;
            store16_out<true>(op, u32x4{v[0], v[1], v[2], v[3]});
            store16_out<true>(op + 1024, u32x4{v[4], v[5], v[6], v[7]});
        }
        __syncthreads();  // rows read and cleared before the next unit's partials
        c += job.gs_c;
        s += job.gs_s;
        if (c >= job.cps) {
            c -= job.cps;
            ++s;
        }
    }
}

// ---------------------------------------------------------------------------
// matapply_small: launches too small to fill the chip with the unit kernels,
// for codes beyond the register kernels (k > 4 or r > 8).  The unit kernels
// give each lane every output row of its slice: a K=20/M=60 stripe of 4 KiB
// (205-byte blocks) is 26 lanes doing 800 coefficient MACs each, ~30-40 us
// in one wave (tools/small_call_probe.py under rocprofv3,
// profiles/r02_small_calls.log).  Here a wave owns one output row (so its
// coefficients are wave-uniform: their tables are scalar loads from the
// bank) and 64 four-byte units of it, and each lane does k MACs with all k
// input loads in flight at once.  Inputs are re-read once per row, from L2
// (host calls stage wide codes through device memory, fec_abi.cpp).  Python
// bytes calls, K=20/M=60: 4 KiB stripe 57-59 -> 25-26 us per encode, 64 KiB
// 77-81 -> 43-52, 256 KiB 111-121 -> 68-79 (profiles/r02_small_calls.log).
// Launch: gs_c = waves per row, gs_s = bytes per unit (4, or 1 when sz < 4),
// cps = units per stripe.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void matapply_small(const MatJob job) {
    const uint32_t wave = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const uint32_t wpr = job.gs_c;
    const uint32_t row = __builtin_amdgcn_readfirstlane(wave / wpr);
    if (row >= job.r) return;
    const uint64_t unit = uint64_t(wave - row * wpr) * 64u + (threadIdx.x & 63u);
    const uint64_t cps = job.cps;
    if (unit >= cps * job.nstripes) return;
    const uint32_t ub = job.gs_s;
    const uint64_t s = unit / cps;
    uint64_t off = (unit - s * cps) * ub;
    // The last unit of a block: shifted back to end at sz (its neighbour
    // stores the same bytes), except when accumulating, where two lanes of
    // different waves would both read-modify-write the overlap: there it
    // takes only its own bytes (nb < 4), one at a time.
    uint32_t nb = ub;
    if (off + ub > job.sz) {
        if (job.accumulate)
            nb = static_cast<uint32_t>(job.sz - off);
        else
            off = job.sz - ub;
    }
    const uint64_t io = s * job.in_sstride + off, oo = s * job.out_sstride + off;
    uint32_t acc = 0;
    if (nb == 4u) {
        // every input load is issued before the first is used: one memory
        // latency per launch instead of one per input
        uint32_t xs[kMaxIn];
#pragma unroll
        for (uint32_t j = 0; j < static_cast<uint32_t>(kMaxIn); ++j)
            if (j < job.k) __builtin_memcpy(&xs[j], job.in[j] + io, 4);
#pragma unroll
        for (uint32_t j = 0; j < static_cast<uint32_t>(kMaxIn); ++j) {
            if (j < job.k) {
                const uint32_t* t = &g_bank.w[uint32_t(job.coef[row * job.k + j]) * 8u];
                const Sel sl = selectors(xs[j]);
                acc = xor3(acc, perm(t[1], t[0], sl.s0), perm(t[3], t[2], sl.s1)) ^ perm(t[4], t[4], sl.s2);
            }
        }
    } else {  // the bytes of a block shorter than 4, or an accumulating launch's tail
        for (uint32_t j = 0; j < job.k; ++j) {
            uint32_t x = 0;
            for (uint32_t q = 0; q < nb; ++q) x |= uint32_t(job.in[j][io + q]) << (8 * q);
            const uint32_t* t = &g_bank.w[uint32_t(job.coef[row * job.k + j]) * 8u];
            const Sel sl = selectors(x);
            acc = xor3(acc, perm(t[1], t[0], sl.s0), perm(t[3], t[2], sl.s1)) ^ perm(t[4], t[4], sl.s2);
        }
    }
    uint8_t* op = job.out[row] + oo;
    if (nb == 4u) {
        if (job.accumulate) {
            uint32_t o;
            __builtin_memcpy(&o, op, 4);
            acc ^= o;
        }
        __builtin_memcpy(op, &acc, 4);
    } else {
        for (uint32_t b = 0; b < nb; ++b) {
            const uint8_t v = static_cast<uint8_t>(acc >> (8 * b));
            op[b] = job.accumulate ? static_cast<uint8_t>(op[b] ^ v) : v;
        }
    }
}

// Launch through hipLaunchKernel itself: hipLaunchKernelGGL (<<<>>>) adds
// __hipPushCallConfiguration / __hipPopCallConfiguration around it, and the
// hipGetLastError after it is one more runtime call; together 0.2-0.35 us of
// host time per launch (tools/host_cost.hip: "launch, 560 B kernarg" against
// "hipLaunchKernel 560 B").  The returned status is the launch's.
template <class J>
hipError_t launch_job(const void* fn, uint32_t grid, uint32_t block, size_t lds, hipStream_t stream, const J& job) {
    void* args[] = {const_cast<J*>(&job)};
    return hipLaunchKernel(fn, dim3(grid), dim3(block), args, lds, stream);
}

// Launches whose unit kernels would run fewer lanes than Config::small_lanes
// (2048 by default) take matapply_small.
hipError_t launch_small(MatJob& job, hipStream_t stream) {
    const uint32_t ub = job.sz >= 4 ? 4u : 1u;
    const uint64_t cps = (job.sz + ub - 1) / ub;
    const uint64_t units = cps * job.nstripes;
    const uint64_t wpr = (units + 63) / 64;
    const uint64_t waves = wpr * job.r;
    if (waves > (1ull << 31)) return hipErrorNotSupported;
    job.cps = static_cast<uint32_t>(cps);
    job.gs_c = static_cast<uint32_t>(wpr);
    job.gs_s = ub;
    const uint32_t grid = static_cast<uint32_t>((waves + kBlock / 64 - 1) / (kBlock / 64));
    return launch_job(reinterpret_cast<const void*>(matapply_small), grid, kBlock, 0, stream, job);
}

// ---------------------------------------------------------------------------
// Dispatch
// ---------------------------------------------------------------------------
typedef void (*KernelFn)(const MatJob);

std::once_flag g_dispatch_once;
int g_num_cu = 256;
// Grid cap of the unit kernels: CUs x 8 x 1024 workgroups, i.e. about one unit
// per lane for any launch this library makes (measured +9 % on 10^6 4 KiB
// stripes against a grid of 16 resident waves per SIMD); a launch past it
// walks grid-stride.
constexpr uint64_t kGridPerCu = 8 * 1024;

// Config::grid_cap (a test hook) lowers a launcher's own cap so that a launch a
// test can afford walks grid-stride; values outside [1, cap) are ignored.  It
// bounds the grid only: the kernel a launch takes is chosen from its units.
uint64_t hooked_grid_cap(uint64_t cap) {
    const uint64_t hook = config().grid_cap;
    return hook >= 1 && hook < cap ? hook : cap;
}
uint64_t unit_grid_cap() { return hooked_grid_cap(uint64_t(g_num_cu) * kGridPerCu); }
// Grid cap of the bit-sliced run-time-data kernels (matapply_bsr in all its
// forms, matapply_bsr_ks, matverify_bsr): CUs x 1024 workgroups.
uint64_t bsr_grid_cap() { return hooked_grid_cap(uint64_t(g_num_cu) * 1024); }

void init_dispatch() {
    int dev = 0;
    if (hipGetDevice(&dev) == hipSuccess) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
            g_num_cu = prop.multiProcessorCount;
    }
}

thread_local const char* t_last_kernel = "";

thread_local uint32_t* t_signal_flag = nullptr;
thread_local uint32_t t_signal_seq = 0;
thread_local bool t_signal_used = false;

// Every public launcher: an unconsumed launch_apply request must not outlive this launch.
void reset_signal() {
    t_signal_flag = nullptr;
    t_signal_used = false;
}

// ---- register kernels (k <= 4, r <= 8) ----------------------------------------
constexpr int kRegK = 4, kRegR = 8;
const char* const kRegNames[kRegK + 1][kRegR + 1] = {
    {},
    {"", "matapply_reg<1,1>", "matapply_reg<1,2>", "matapply_reg<1,3>", "matapply_reg<1,4>", "matapply_reg<1,5>",
     "matapply_reg<1,6>", "matapply_reg<1,7>", "matapply_reg<1,8>"},
    {"", "matapply_reg<2,1>", "matapply_reg<2,2>", "matapply_reg<2,3>", "matapply_reg<2,4>", "matapply_reg<2,5>",
     "matapply_reg<2,6>", "matapply_reg<2,7>", "matapply_reg<2,8>"},
    {"", "matapply_reg<3,1>", "matapply_reg<3,2>", "matapply_reg<3,3>", "matapply_reg<3,4>", "matapply_reg<3,5>",
     "matapply_reg<3,6>", "matapply_reg<3,7>", "matapply_reg<3,8>"},
    {"", "matapply_reg<4,1>", "matapply_reg<4,2>", "matapply_reg<4,3>", "matapply_reg<4,4>", "matapply_reg<4,5>",
     "matapply_reg<4,6>", "matapply_reg<4,7>", "matapply_reg<4,8>"}};

const char* const kRowsNames[kRegK + 1][kRegR + 1] = {
    {},
    {"", "matapply_rows<1,1>", "matapply_rows<1,2>", "matapply_rows<1,3>", "matapply_rows<1,4>",
     "matapply_rows<1,5>", "matapply_rows<1,6>", "matapply_rows<1,7>", "matapply_rows<1,8>"},
    {"", "matapply_rows<2,1>", "matapply_rows<2,2>", "matapply_rows<2,3>", "matapply_rows<2,4>",
     "matapply_rows<2,5>", "matapply_rows<2,6>", "matapply_rows<2,7>", "matapply_rows<2,8>"},
    {"", "matapply_rows<3,1>", "matapply_rows<3,2>", "matapply_rows<3,3>", "matapply_rows<3,4>",
     "matapply_rows<3,5>", "matapply_rows<3,6>", "matapply_rows<3,7>", "matapply_rows<3,8>"},
    {"", "matapply_rows<4,1>", "matapply_rows<4,2>", "matapply_rows<4,3>", "matapply_rows<4,4>",
     "matapply_rows<4,5>", "matapply_rows<4,6>", "matapply_rows<4,7>", "matapply_rows<4,8>"}};

// Output store policy of the register kernels: nt sc1 (written through the L2
// at device scope) for single-stripe launches -- a few long rows, where it measured faster: the
// cfg2 64 MiB K=3/M=10 stripe, encode 68.5 -> 69.1-69.9 % of HBM from cold
// caches, secondary decode 65.6 -> 68.0 %, bench value +1.2-1.5 % -- and nt for
// batches of many stripes, where nt sc1 measured slower (256 x 1 MiB
// object-major 69.5 -> 67.7 %, 10^6 x 4 KiB -1 %; tools/ab_store.sh,
// profiles/r02_store_ab.log; copy-walk probe: tools/mb_cold.exe tail).
// Fill a register kernel's argument block for `a`; returns its grid (0: more
// units than one launch walks -- the caller splits).  rows: matapply_rows'
// one-wave-per-stripe walk.
template <int K, int R>
uint32_t fill_regjob(const ApplySpec& a, RegJob<K, R>& job, bool rows) {
    job.sz = a.sz;
    job.in_sstride = a.in_sstride;
    job.out_sstride = a.out_sstride;
    job.nstripes = static_cast<uint32_t>(a.nstripes);
    job.done_flag = nullptr;
    job.done_seq = 0;
    job.pad_ = 0;
    for (int j = 0; j < K; ++j) job.in[j] = a.in[j];
    for (int i = 0; i < R; ++i) job.out[i] = a.out[i];
    for (int i = 0; i < R; ++i)
        for (int j = 0; j < K; ++j) host_tab(&job.tab[(i * K + j) * 5], a.coef[size_t(i) * a.coef_stride + j]);
    const uint64_t cps = (a.sz + kChunk - 1) / kChunk;
    if (cps * a.nstripes >= (1ull << 32) - (1ull << 24)) return 0;
    job.cps = static_cast<uint32_t>(cps);
    // one unit per lane up to the grid cap; beyond it a grid-stride loop
    const uint64_t lanes = rows ? a.nstripes * 64u : cps * a.nstripes;  // rows: one wave per stripe
    const uint64_t need = (lanes + kBlock - 1) / kBlock;
    const uint64_t cap = unit_grid_cap();
    const uint32_t grid = static_cast<uint32_t>(need < cap ? need : cap);
    const uint64_t gstride = uint64_t(grid) * kBlock;
    job.gs_s = static_cast<uint32_t>(gstride / cps);
    job.gs_c = static_cast<uint32_t>(gstride % cps);
    return grid;
}

bool rows_shape(const ApplySpec& a) { return a.sz > kRowsMin && a.sz <= kRowsMax && a.nstripes >= 64; }

template <int K, int R>
hipError_t launch_reg(const ApplySpec& a, hipStream_t stream, uint32_t* sig) {
    // many outputs: the prefetching walk (K=3/M=10 encode 6.17 -> 6.41 TB/s,
    // tools/mb_encode.exe; no gain for the 3-row decode)
    constexpr bool kPrefetch = reg_prefetch(R);
    // more table dwords than the SGPRs hold next to the pointers: read them
    // where they are used (K=3/M=10 encode 35.9 -> 33.6 us, tools/mb_encode.exe
    // variant "PF AL"; the 3-row decode is unchanged either way)
    constexpr bool kArgLoad = reg_argload(K, R);
    RegJob<K, R> job;
    const bool rows = rows_shape(a);
    const uint32_t grid = fill_regjob<K, R>(a, job, rows);
    if (!grid) return hipErrorInvalidValue;  // the caller splits
    void (*fn)(const RegJob<K, R>);
    if (rows) {
        fn = matapply_rows<K, R, kArgLoad>;
        t_last_kernel = kRowsNames[K][R];
    } else {
        // Single stripes store nt sc1 -- unless an output row starts off a
        // 16-byte line: its 16-byte stores straddle two lines, and written
        // through (sc1) each straddling store costs a partial-line write; nt
        // alone lets the L2 merge the halves.  K=3/M=10 64 MiB, outputs at 6
        // (mod 16): nt sc1 47.2 us, nt 41.6-42.0 us, aligned 39.6
        // (tools/misaligned_bench.py, profiles/r04_misaligned_ab.json; staging
        // the rows through LDS to store aligned lines measured 56-62 us, and
        // assembling them across lanes with DPP 90 us).
        bool ma = false;
        for (int i = 0; i < R; ++i) ma = ma || (reinterpret_cast<uintptr_t>(a.out[i]) & 15u) != 0;
        fn = a.nstripes == 1 && !ma ? matapply_reg<K, R, 3, kPrefetch, kArgLoad>
                                    : matapply_reg<K, R, 0, kPrefetch, kArgLoad>;
        t_last_kernel = kRegNames[K][R];
        if (sig && grid == 1) {  // one workgroup: it signals its own completion
            job.done_flag = sig;
            job.done_seq = t_signal_seq;
            t_signal_used = true;
        }
#if ZFEC_REG_ONE
        // one stripe, every unit has its own lane, no byte tail, no signal:
        // the straight-line form (reg_body_one)
        else if (a.nstripes == 1 && a.sz >= kChunk && uint64_t(grid) * kBlock >= job.cps) {
            constexpr int kOne = kArgLoad && ZFEC_REG_TPIPE ? 2 : 1;
            fn = !ma ? matapply_reg<K, R, 3, kPrefetch, kArgLoad, kOne> : matapply_reg<K, R, 0, kPrefetch, kArgLoad, kOne>;
        }
#endif
    }
    return launch_job(reinterpret_cast<const void*>(fn), grid, kBlock, 0, stream, job);
}

typedef hipError_t (*RegLaunch)(const ApplySpec&, hipStream_t, uint32_t*);

template <int K, int... R>
constexpr std::array<RegLaunch, kRegR + 1> reg_row(std::integer_sequence<int, R...>) {
    return {{nullptr, launch_reg<K, R + 1>...}};
}

const std::array<RegLaunch, kRegR + 1> g_reg_launch[kRegK + 1] = {
    {}, reg_row<1>(std::make_integer_sequence<int, kRegR>()), reg_row<2>(std::make_integer_sequence<int, kRegR>()),
    reg_row<3>(std::make_integer_sequence<int, kRegR>()), reg_row<4>(std::make_integer_sequence<int, kRegR>())};

// ---- paired register launches (matapply_pair) ------------------------------------
char g_pair_names[kRegK + 1][kRegR + 1][kRegR + 1][32];

template <int K, int RA, int RB>
hipError_t launch_pair(const ApplySpec& a, const ApplySpec& b, hipStream_t stream) {
    PairJob<K, RA, RB> job;
    const uint32_t ga = fill_regjob<K, RA>(a, job.a, false), gb = fill_regjob<K, RB>(b, job.b, false);
    if (!ga || !gb || uint64_t(ga) + gb >= (1ull << 31)) return hipErrorNotSupported;
    job.blocks_a = ga;
    job.pad_[0] = job.pad_[1] = job.pad_[2] = 0;
    // the register kernels' store policy, single-stripe (nt sc1) only when both are
    const bool sc1 = a.nstripes == 1 && b.nstripes == 1;
    void (*fn)(const PairJob<K, RA, RB>) = sc1 ? matapply_pair<K, RA, RB, 3> : matapply_pair<K, RA, RB, 0>;
    t_last_kernel = g_pair_names[K][RA][RB];
    return launch_job(reinterpret_cast<const void*>(fn), ga + gb, kBlock, 0, stream, job);
}

typedef hipError_t (*PairLaunch)(const ApplySpec&, const ApplySpec&, hipStream_t);
typedef std::array<PairLaunch, kRegR + 1> PairRow;

template <int K, int RA, int RB>
constexpr PairLaunch pair_entry() {
    if constexpr (RB <= K && RB <= RA)
        return launch_pair<K, RA, RB>;
    else
        return nullptr;
}

template <int K, int RA, int... RB>
constexpr PairRow pair_row(std::integer_sequence<int, RB...>) {
    return {{nullptr, pair_entry<K, RA, RB + 1>()...}};
}

template <int K, int... RA>
constexpr std::array<PairRow, kRegR + 1> pair_plane(std::integer_sequence<int, RA...>) {
    return {{PairRow{}, pair_row<K, RA + 1>(std::make_integer_sequence<int, kRegR>())...}};
}

const std::array<PairRow, kRegR + 1> g_pair_launch[kRegK + 1] = {
    {}, pair_plane<1>(std::make_integer_sequence<int, kRegR>()), pair_plane<2>(std::make_integer_sequence<int, kRegR>()),
    pair_plane<3>(std::make_integer_sequence<int, kRegR>()), pair_plane<4>(std::make_integer_sequence<int, kRegR>())};

// ---- per-RT variant tables -------------------------------------------------------
// f(integral_constant<int, I>) for I = 1 .. N: fills a table of kernels
// instantiated per row-tile height.
template <class F, int... I>
void for_each_rt(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I + 1>{}), ...);
}
template <int N, class F>
void for_each_rt(F&& f) {
    for_each_rt(f, std::make_integer_sequence<int, N>());
}

// A variant's name as matapply_last_kernel() reports it: "kernel<RT tags>".
typedef char KName[40];
void kname(KName& dst, const char* kernel, int rt, const char* tags) {
    snprintf(dst, sizeof dst, "%s<%d%s>", kernel, rt, tags);
}

// ---- table kernels (matapply_lds, k <= 32, r <= 48) ----------------------------
struct LdsVariant {
    KernelFn fn;
    const char* name;
    int chunk;     // bytes per unit (a lane's slice of one block)
    int pad_tile;  // kTilesPadded: rows per tile (the LDS table is padded to whole tiles); 0: ragged
};

// Padded-tile variants by tile height: 1-8 rows in one tile (r <= 8), 9-20
// rows for wider codes split into ceil(r/20) near-equal tiles.
constexpr int kMaxTile = 20;
KName g_pad_names[kMaxTile + 1];
LdsVariant g_lds_pad[kMaxTile + 1];
// measured (tools/mb_encode.exe MB_AB, interleaved medians): k <= 4
// (memory-bound) takes 16 bytes per lane in ragged 8-row tiles; wider codes
// take 8 bytes per lane in padded tiles (no per-row branches), as few tiles as
// 20-row register tiles allow (inputs are re-read per tile)
const LdsVariant g_lds_fewin{matapply_lds<false, true, 8, 4, 4>, "matapply_lds<8,4,4>", 16, 0};
const LdsVariant g_lds_acc{matapply_lds<true, false, 16, 2, 2>, "matapply_lds<16,2,2,acc>", 8, 0};

void fill_pad() {
    for_each_rt<kMaxTile>([](auto rt) {
        constexpr int RT = decltype(rt)::value;
        constexpr int G = (RT <= 4 || RT == 8) ? 4 : 2;  // input group size: measured per tile height
        kname(g_pad_names[RT], "matapply_lds", RT, G == 4 ? ",2,4,pad" : ",2,2,pad");
        g_lds_pad[RT] = LdsVariant{matapply_lds<false, true, RT, 2, G, kTilesPadded>, g_pad_names[RT], 8, RT};
    });
}

std::once_flag g_pad_once;

const LdsVariant& pick_lds(uint32_t k, uint32_t r, bool acc) {
    std::call_once(g_pad_once, fill_pad);
    if (acc) return g_lds_acc;
    if (k <= 4) return g_lds_fewin;
    const uint32_t tiles = (r + kMaxTile - 1) / kMaxTile;
    return g_lds_pad[(r + tiles - 1) / tiles];
}

// The header of a unit-walk job (any job type with these six fields).
template <class J>
void fill_header(J& job, const ApplySpec& a) {
    job.sz = a.sz;
    job.in_sstride = a.in_sstride;
    job.out_sstride = a.out_sstride;
    job.nstripes = static_cast<uint32_t>(a.nstripes);
    job.k = a.k;
    job.r = a.r;
}

// The grid-stride unit walk of a launch over `units` units, cps per stripe,
// into any job with the three walk fields: at most `cap` workgroups, each
// taking `per_wg` units per step (kBlock lanes for matapply_lds, one unit for
// the bit-sliced kernels); returns the grid.
template <class J>
uint32_t fill_stride(J& job, uint64_t cps, uint64_t units, uint64_t cap, uint32_t per_wg = 1) {
    const uint64_t need = (units + per_wg - 1) / per_wg;
    const uint32_t grid = static_cast<uint32_t>(need < cap ? need : cap);
    const uint64_t gstride = uint64_t(grid) * per_wg;
    job.cps = static_cast<uint32_t>(cps);
    job.gs_s = static_cast<uint32_t>(gstride / cps);
    job.gs_c = static_cast<uint32_t>(gstride % cps);
    return grid;
}

// Both: the header and walk of a one-unit-per-workgroup launch.
template <class J>
uint32_t fill_units(J& job, const ApplySpec& a, uint64_t cps, uint64_t units, uint64_t cap) {
    fill_header(job, a);
    return fill_stride(job, cps, units, cap);
}

// (the walk fields are the launcher's: fill_stride, launch_small)
void fill_matjob(const ApplySpec& a, MatJob& job) {
    fill_header(job, a);
    job.accumulate = a.accumulate;
    job.pad_ = 0;
    for (uint32_t j = 0; j < a.k; ++j) job.in[j] = a.in[j];
    for (uint32_t i = 0; i < a.r; ++i) job.out[i] = a.out[i];
}

void fill_coef(const ApplySpec& a, MatJob& job) {
    for (uint32_t i = 0; i < a.r; ++i) std::memcpy(&job.coef[i * a.k], a.coef + size_t(i) * a.coef_stride, a.k);
}

hipError_t launch_lds(const ApplySpec& a, hipStream_t stream) {
    const LdsVariant& v = pick_lds(a.k, a.r, a.accumulate);
    const uint64_t cps = (a.sz + v.chunk - 1) / v.chunk;
    const uint64_t total = cps * a.nstripes;
    if (total >= (1ull << 32) - (1ull << 24)) return hipErrorInvalidValue;  // the caller splits larger jobs
    MatJob job;
    fill_matjob(a, job);
    fill_coef(a, job);
    const size_t rows = v.pad_tile ? (a.r + v.pad_tile - 1) / v.pad_tile * v.pad_tile : a.r;
    const size_t lds = size_t(a.k) * rows * 32;
    const uint32_t grid = fill_stride(job, cps, total, unit_grid_cap(), kBlock);
    t_last_kernel = v.name;
    return launch_job(reinterpret_cast<const void*>(v.fn), grid, kBlock, lds, stream, job);
}

// ---- matapply_bsg dispatch ------------------------------------------------------
// Rows per wave: the smallest instantiated RT >= ceil(r / 4).
constexpr int kBsgRT[] = {1, 2, 3, 4, 5, 6, 8, 10, 12};
constexpr int kBsgNumRT = sizeof(kBsgRT) / sizeof(kBsgRT[0]);
constexpr uint32_t kBsgMaxRows = 4u * 12u;

struct BsgVariant {
    const void* fn_karg = nullptr;  // matapply_bsg<RT, false, MatJob>
    const void* fn_tbl = nullptr;   // matapply_bsg<RT, true, BsgTblJob>
    KName name = "";
    KName name_tbl = "";
    int blocks_per_cu = 1;          // resident workgroups per CU (occupancy API), set once
};
BsgVariant g_bsg_var[kBsgNumRT];
std::once_flag g_bsg_once;
std::atomic<int> g_generic{-1};

void fill_bsg() {
    for_each_rt<kBsgNumRT>([](auto i) {
        constexpr int RT = kBsgRT[decltype(i)::value - 1];
        BsgVariant& v = g_bsg_var[decltype(i)::value - 1];
        v.fn_karg = reinterpret_cast<const void*>(matapply_bsg<RT, false, MatJob>);
        v.fn_tbl = reinterpret_cast<const void*>(matapply_bsg<RT, true, BsgTblJob>);
        kname(v.name, "matapply_bsg", RT, ",2");
        kname(v.name_tbl, "matapply_bsg", RT, ",2,tbl");
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, v.fn_karg, 256, kBsgPhase * kBsgSlotBytes) ==
                hipSuccess &&
            nb > 0)
            v.blocks_per_cu = nb;
        else
            (void)hipGetLastError();
    });
}

bool bsg_shape_ok(uint32_t k, uint32_t r, uint64_t sz) {
    // k * r >= 24, not a register-kernel shape; past 32 inputs (the table form)
    // up to 256 rows in one launch, otherwise one group of <= 48
    const uint32_t rmax = k > static_cast<uint32_t>(kMaxIn) ? 256u : kBsgMaxRows;
    return generic_mode() != 0 && sz >= kBsgChunk && k >= 1 && k <= static_cast<uint32_t>(kMaxWideIn) && r >= 1 &&
           r <= rmax && k * r >= 24 && !(k <= 4 && r <= 8);
}

// Events that only tell the host when a table slot's readers have finished
// (hipEventSynchronize before the slot is rewritten, hipStreamWaitEvent for
// another stream of the same device): no system-scope release, which would
// write the L2's dirty lines back at every launch that records one.
constexpr unsigned kSlotEventFlags = hipEventDisableTiming | hipEventDisableSystemFence;

// A staging slot: pinned host memory, its device twin filled by stream-ordered
// copies, and an event recorded after the slot's last reader and waited for
// before the slot is rewritten.
struct Slot {
    uint8_t* dev = nullptr;
    uint8_t* host = nullptr;
    hipEvent_t ev = nullptr;
    bool busy = false;
    hipError_t alloc(size_t bytes) {
        hipError_t e = hipMalloc(&dev, bytes);
        if (e != hipSuccess) return e;
        if ((e = hipHostMalloc(&host, bytes, hipHostMallocDefault)) != hipSuccess) {
            (void)hipFree(dev);
            dev = nullptr;
        }
        return e;
    }
    void free_mem() {
        if (dev) (void)hipFree(dev);
        if (host) (void)hipHostFree(host);
        dev = host = nullptr;
    }
    hipError_t event() { return ev ? hipSuccess : hipEventCreateWithFlags(&ev, kSlotEventFlags); }
    void drop_event() {
        if (ev) (void)hipEventSynchronize(ev), (void)hipEventDestroy(ev);
    }
    hipError_t wait() {  // until the slot's last reader has finished
        if (busy) {
            const hipError_t e = hipEventSynchronize(ev);
            if (e != hipSuccess) return e;
        }
        busy = false;
        return hipSuccess;
    }
    hipError_t record(hipStream_t stream) {  // after the slot's last reader
        const hipError_t e = hipEventRecord(ev, stream);
        if (e == hipSuccess) busy = true;
        return e;
    }
};

// N slots of BYTES each in one allocation, made with their events on first
// use: slot 0 owns the memory, the others point into it.
template <int N, size_t BYTES>
struct FixedRing {
    static constexpr int kSlots = N;
    static constexpr size_t kSlotBytes = BYTES;
    Slot slot[N];
    unsigned next = 0;
    hipError_t init() {
        if (slot[0].dev) return hipSuccess;
        hipError_t e = slot[0].alloc(N * BYTES);
        if (e != hipSuccess) return e;
        for (int i = 1; i < N; ++i) {
            slot[i].dev = slot[0].dev + i * BYTES;
            slot[i].host = slot[0].host + i * BYTES;
        }
        for (Slot& s : slot)
            if ((e = s.event()) != hipSuccess) return e;
        return hipSuccess;
    }
    void release() {
        for (Slot& s : slot) s.drop_event();
        slot[0].free_mem();
    }
};

// The calling thread's ring of each device; a ring is released on its own
// device when the thread exits.
template <class R>
struct PerDevice {
    std::unordered_map<int, R> dev;
    hipError_t here(R** ring) {
        int id = 0;
        const hipError_t e = hipGetDevice(&id);
        if (e == hipSuccess) *ring = &dev[id];
        return e;
    }
    ~PerDevice() {
        for (auto& kv : dev) {
            int cur = 0;
            if (hipGetDevice(&cur) != hipSuccess || hipSetDevice(kv.first) != hipSuccess) continue;
            kv.second.release();
            (void)hipSetDevice(cur);
        }
    }
};

// Device-side argument tables of wide matapply_bsg launches: a slot is reused
// once the event recorded after its last launch has completed.
typedef FixedRing<8, (size_t(160) << 10)> TableRing;  // k, r <= 256 with 64 row groups of 4
thread_local PerDevice<TableRing> t_rings;

hipError_t ring_slot(Slot** slot) {
    TableRing* t = nullptr;
    hipError_t e = t_rings.here(&t);
    if (e != hipSuccess || (e = t->init()) != hipSuccess) return e;
    Slot& s = t->slot[t->next++ % TableRing::kSlots];
    if ((e = s.wait()) != hipSuccess) return e;  // its last launch has read it
    *slot = &s;
    return hipSuccess;
}

// matapply_bsg launch (the table form declines under graph capture: stream_capturing).
hipError_t launch_bsg(const ApplySpec& a, hipStream_t stream) {
    std::call_once(g_bsg_once, fill_bsg);
    const uint32_t k = a.k, r = a.r;
    const uint64_t cps = (a.sz + kBsgChunk - 1) / kBsgChunk;
    const uint64_t units = cps * a.nstripes;
    // Rows per wave: the smallest instantiated RT >= ceil(r / 4), at most 12
    // (48 rows per group of the walk).  A launch with fewer than ~4 workgroups
    // per CU of (unit, row group) work takes smaller row groups: each group's
    // workgroups rebuild the inputs' combinations, which costs less than idle
    // CUs (a 64 MiB stripe of a 128/256 code is 128 units of 4 KiB).  The
    // shrinking stops at RT 2: one row per wave re-reads every input per 4
    // rows, and measured slower than half-idle CUs (profiles/r03_bsg_wgs.json:
    // 200/256 at RT 2 0.207 ms, RT 1 0.278 ms; 128/256 at RT 4 0.249 ms, RT 10
    // 0.351 ms, RT 2 0.312 ms).
    constexpr uint32_t kBsgWgsPerCu = 4;
    const uint32_t need_rt = (r + 3) / 4;
    int ri = 0;
    while (ri + 1 < kBsgNumRT && kBsgRT[ri] < static_cast<int>(need_rt)) ++ri;
    const uint64_t target = uint64_t(kBsgWgsPerCu) * static_cast<uint64_t>(g_num_cu);
    auto groups_of = [&](int i) { return (r + 4u * kBsgRT[i] - 1) / (4u * kBsgRT[i]); };
    while (ri > 1 && units * groups_of(ri) < target) --ri;
    const uint32_t ngroups = groups_of(ri);
    const BsgVariant& v = g_bsg_var[ri];
    // coefficients in the kernel's walk order: group g, wave w, phase f at
    // ((g * 4 + w) * nph + f) * PB, (js, rr) in order: row g * 4 * RT + w + 4 * rr
    // of input 2 * f + js
    const uint32_t RT = static_cast<uint32_t>(kBsgRT[ri]), P = kBsgPhase;
    const uint32_t PB = (P * RT + 3) / 4 * 4, nph = (k + P - 1) / P;
    const uint32_t walk = ngroups * 4u * nph * PB;
    auto fill_walk = [&](uint8_t* cf) {
        std::memset(cf, 0, walk);
        for (uint32_t g = 0; g < ngroups; ++g)
            for (uint32_t w = 0; w < 4; ++w)
                for (uint32_t f = 0; f < nph; ++f)
                    for (uint32_t js = 0; js < P; ++js)
                        for (uint32_t rr = 0; rr < RT; ++rr) {
                            const uint32_t i = g * 4 * RT + w + 4 * rr, j = P * f + js;
                            if (i < r && j < k && w + 4 * rr < 4 * RT)
                                cf[((g * 4 + w) * nph + f) * PB + js * RT + rr] =
                                    a.coef[size_t(i) * a.coef_stride + j];
                        }
    };
    const size_t lds = size_t(P) * kBsgSlotBytes;
    const uint64_t vunits = units * ngroups;
    if (vunits >= (1ull << 32) - (1ull << 24)) return hipErrorInvalidValue;
    const uint64_t cap = hooked_grid_cap(uint64_t(g_num_cu) * v.blocks_per_cu * 8);
    if (ngroups == 1 && k <= static_cast<uint32_t>(kMaxIn) && r <= static_cast<uint32_t>(kMaxOut) &&
        walk <= static_cast<uint32_t>(kMaxCoef)) {
        MatJob job;
        fill_matjob(a, job);
        fill_walk(job.coef);
        t_last_kernel = v.name;
        return launch_job(v.fn_karg, fill_stride(job, cps, vunits, cap), 256, lds, stream, job);
    }
    // pointers and coefficients in a device-side table
    if (stream_capturing(stream)) return hipErrorNotSupported;
    const size_t bytes = 8 * size_t(k + r) + walk;
    if (bytes > TableRing::kSlotBytes) return hipErrorNotSupported;
    Slot* slot = nullptr;
    hipError_t e = ring_slot(&slot);
    if (e != hipSuccess) return e;
    uint8_t* h = slot->host;
    uint8_t* d = slot->dev;
    std::memcpy(h, a.in, 8 * size_t(k));
    std::memcpy(h + 8 * size_t(k), a.out, 8 * size_t(r));
    fill_walk(h + 8 * size_t(k + r));
    if ((e = hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, stream)) != hipSuccess) return e;
    BsgTblJob job;
    const uint32_t grid = fill_units(job, a, cps, vunits, cap);
    job.ngroups = ngroups;
    job.pad_ = 0;
    job.table = d;
    if ((e = launch_job(v.fn_tbl, grid, 256, lds, stream, job)) != hipSuccess) return e;
    if ((e = slot->record(stream)) != hipSuccess) return e;
    t_last_kernel = v.name_tbl;
    return hipSuccess;
}

// ---- matapply_bsr dispatch ------------------------------------------------------
// Whether an nw-wave LDS-phase launch shares the inputs' 30 combinations through
// LDS (built once per workgroup, phases of one input per wave) instead of the 8
// planes (the 22 multi-plane combinations rebuilt by every wave): with 8 waves,
// where rebuilding is 8x the work (128/256 0.130 -> 0.122 ms per 64 MiB stripe);
// with 2 or 4 the short phases cost more than the XORs saved (cfg4's first-seen
// 20-row decode 0.439 -> 0.474 ms, 30/70 0.070 -> 0.074; profiles/r05_bsr_cmb_ab.json;
// on DMA-staged phases 0.419 -> 0.428 and 0.065 -> 0.067, r05_lds_dma_ab.json).
// ZFEC_BSR_CMB_MIN_NW: the least waves per workgroup that share combinations
// (default 8; the A/B knob of tools/ab_build.sh)
#ifndef ZFEC_BSR_CMB_MIN_NW
#define ZFEC_BSR_CMB_MIN_NW 8
#endif
bool bsr_cmb(uint32_t nw) { return nw >= ZFEC_BSR_CMB_MIN_NW; }

// LDS of an nw-wave LDS-phase launch over k inputs: one phase of combinations
// and its raw staging, or two phases of planes (one when a single phase holds
// all k).
size_t bsr_lds_bytes(uint32_t k, uint32_t nw, bool cmb) {
    const uint32_t ph = cmb ? bsr_cmb_phase(nw) : bsr_db_phase(nw);
    if (cmb) return size_t(k < ph ? k : ph) * (bsr_in_bytes<true>() + bsr_in_bytes<false>());  // + raw staging
    return size_t(k <= ph ? k : 2 * ph) * bsr_in_bytes<false>();
}

// nw = ceil(r / 10) waves, one per row tile of <= RT = ceil(r / nw) rows.
struct BsrVariant {
    const void* fn = nullptr;
    const void* fn_cmb = nullptr;  // combination-sharing form (bsr_cmb)
    const void* fn_solo = nullptr;
    KName name = "";
    KName name_cmb = "";
    KName name_solo = "";
};
BsrVariant g_bsr_var[kBsrMaxRows + 1];
std::once_flag g_bsr_once;

void fill_bsr() {
    for_each_rt<kBsrMaxRows>([](auto rt) {
        constexpr int RT = decltype(rt)::value;
        BsrVariant& v = g_bsr_var[RT];
        v.fn = reinterpret_cast<const void*>(matapply_bsr<RT, false, false, BsrJob>);
        v.fn_cmb = reinterpret_cast<const void*>(matapply_bsr<RT, false, true, BsrJob>);
        v.fn_solo = reinterpret_cast<const void*>(matapply_bsr_solo<RT>);
        kname(v.name, "matapply_bsr", RT, ",lds");
        kname(v.name_cmb, "matapply_bsr", RT, ",lds,cmb");
        kname(v.name_solo, "matapply_bsr", RT, "");
    });
}

// The address of the routine table on each device, read by bsr_table_probe
// (the host writes every coefficient's routine address into the launches'
// arguments).  Only a successful probe is latched: a failed one (stream,
// pinned buffer, launch or sync error) is reported on stderr under
// ZFEC_HIP_JIT_VERBOSE and retried by a later launch, up to kBsrProbeTries per
// device; until one succeeds the device gets no matapply_bsr launches
// (launch_apply hands them to matapply_bsg).
constexpr int kBsrMaxDevices = 64;
constexpr int kBsrProbeTries = 3;
struct BsrBase {
    std::mutex mu;
    std::atomic<uint64_t> addr{0};  // nonzero: the probe succeeded
    int tries = 0;
};
BsrBase g_bsr_base[kBsrMaxDevices];

hipError_t bsr_probe(uint64_t* addr) {
    hipStream_t st = nullptr;
    hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    if (e != hipSuccess) return e;
    uint64_t* h = nullptr;
    if ((e = hipHostMalloc(reinterpret_cast<void**>(&h), sizeof(uint64_t), hipHostMallocDefault)) == hipSuccess) {
        *h = 0;
        hipLaunchKernelGGL(bsr_table_probe, dim3(1), dim3(64), 0, st, h);
        if ((e = hipGetLastError()) == hipSuccess && (e = hipStreamSynchronize(st)) == hipSuccess)
            *addr = *h;
        (void)hipHostFree(h);
    }
    (void)hipStreamDestroy(st);
    return e;
}

hipError_t bsr_routine_base(uint64_t* base, hipStream_t stream) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kBsrMaxDevices) return hipErrorNotSupported;
    BsrBase& b = g_bsr_base[dev];
    uint64_t a = b.addr.load(std::memory_order_acquire);
    if (!a) {
        // the probe synchronises a stream of its own: not while the launch
        // stream is being captured into a graph (the launch declines; a later one probes)
        if (stream_capturing(stream)) return hipErrorNotSupported;
        std::lock_guard<std::mutex> g(b.mu);
        a = b.addr.load(std::memory_order_acquire);
        if (!a && b.tries < kBsrProbeTries) {
            ++b.tries;
            uint64_t got = 0;
            const hipError_t e = bsr_probe(&got);
            if (e == hipSuccess && got) {
                b.addr.store(got, std::memory_order_release);
                a = got;
            } else {
                (void)hipGetLastError();
                if (getenv("ZFEC_HIP_JIT_VERBOSE"))
                    fprintf(stderr, "zfec_hip: routine-table probe on device %d failed (try %d of %d): %s\n", dev,
                            b.tries, kBsrProbeTries, e == hipSuccess ? "address 0" : hipGetErrorString(e));
            }
        }
        if (!a) return hipErrorNotSupported;
    }
    *base = a;
    return hipSuccess;
}

// Routine addresses in a bsr kernel's walk order, [group][wave][input][rt]:
// group g holds rows g*r/ng .. (g+1)*r/ng - 1, split over its nw waves as the
// kernels split them; routine 0 (which only returns) past a wave's rows.  The
// first input a wave walks -- input 0, or with the inputs split over `split`
// waves (the ks form) inputs s*k/split -- calls the "set" routines, which
// write the rows instead of adding to them (the kernels do not zero their
// accumulators).  False if a wave would hold more than rt rows (the kernel
// would drop them).
bool fill_bsr_addrs(uint64_t* dst, const ApplySpec& a, uint64_t base, uint32_t ng, uint32_t nw, uint32_t rt,
                    uint32_t split) {
    const uint32_t k = a.k, r = a.r;
    std::vector<uint8_t> first(k, 0);
    for (uint32_t w = 0; w < split; ++w)
        if (w * k / split < (w + 1) * k / split) first[w * k / split] = 1;
    for (uint32_t g = 0; g < ng; ++g) {
        const uint32_t gr0 = g * r / ng, grn = (g + 1) * r / ng - gr0;
        for (uint32_t w = 0; w < nw; ++w) {
            const uint32_t r0 = gr0 + w * grn / nw, rows = gr0 + (w + 1) * grn / nw - r0;
            if (rows > rt) return false;
            uint64_t* d = dst + size_t(g * nw + w) * k * rt;
            for (uint32_t j = 0; j < k; ++j) {
                const uint64_t tb = base + (first[j] ? kBsrSetBase : 0u);
                for (uint32_t rr = 0; rr < rt; ++rr)  // (row slot rr's table in the slots form)
                    d[size_t(j) * rt + rr] = tb + uint64_t(kBsrSlotStride) * rr +
                                             uint64_t(kBsrStride) * (rr < rows ? a.coef[size_t(r0 + rr) * a.coef_stride + j] : 0u);
            }
        }
    }
    return true;
}

// Device-side routine-address tables of the table forms, kept per (thread,
// device) by matrix and layout: a launch whose table is held reads it as is
// (its block pointers travel in the kernel arguments), so a matrix's table is
// copied to the device by its first launch only.  Copying the table per launch
// cost 19 us ahead of each 0.10 ms 200/256 launch (90 KB of addresses).  Slots
// are reused round-robin once the launches that read them have finished (an
// event per slot); a launch on another stream than the slot's last one is
// ordered after it (hipStreamWaitEvent), so one event covers every reader.
struct BsrTblCache : FixedRing<8, (size_t(160) << 10)> {
    // (a slot's event: recorded after the last launch that read the slot, and its upload)
    hipStream_t last[kSlots] = {};
    uint32_t dims[kSlots][6] = {};  // k, r, ng, nw, rt, split of the table held (k == 0: empty)
    std::vector<uint8_t> coef[kSlots];
};
thread_local PerDevice<BsrTblCache> t_bsr_tbl;

struct BsrTblRef {
    BsrTblCache* c = nullptr;
    unsigned slot = 0;
    const uint64_t* dev = nullptr;
};

hipError_t bsr_table_done(const BsrTblRef& t, hipStream_t stream) {
    const hipError_t e = t.c->slot[t.slot].record(stream);
    if (e == hipSuccess) t.c->last[t.slot] = stream;
    return e;
}

// The device-side address table of a (matrix, layout) for a launch on `stream`
// (ng row groups of nw waves of rt rows, inputs split over `split` waves),
// uploaded on a miss; the caller
// launches, then calls bsr_table_done.
hipError_t bsr_addr_table(const ApplySpec& a, hipStream_t stream, uint64_t base, uint32_t ng, uint32_t nw, uint32_t rt,
                          uint32_t split, BsrTblRef* ref) {
    const uint32_t k = a.k, r = a.r;
    const size_t n = size_t(ng) * nw * k * rt;
    if (n * 8 > BsrTblCache::kSlotBytes || stream_capturing(stream)) return hipErrorNotSupported;
    BsrTblCache* cp = nullptr;
    hipError_t e = t_bsr_tbl.here(&cp);
    if (e != hipSuccess || (e = cp->init()) != hipSuccess) return e;
    BsrTblCache& c = *cp;
    thread_local std::vector<uint8_t> m;  // the matrix, row-major: the key with the layout
    m.resize(size_t(r) * k);
    for (uint32_t i = 0; i < r; ++i) std::memcpy(&m[size_t(i) * k], a.coef + size_t(i) * a.coef_stride, k);
    const uint32_t dims[6] = {k, r, ng, nw, rt, split};
    for (unsigned i = 0; i < BsrTblCache::kSlots; ++i) {
        if (std::memcmp(c.dims[i], dims, sizeof dims) != 0 || c.coef[i] != m) continue;
        if (c.slot[i].busy && c.last[i] != stream && (e = hipStreamWaitEvent(stream, c.slot[i].ev, 0)) != hipSuccess)
            return e;
        *ref = BsrTblRef{&c, i, reinterpret_cast<const uint64_t*>(c.slot[i].dev)};
        return hipSuccess;
    }
    const unsigned i = c.next++ % BsrTblCache::kSlots;
    if ((e = c.slot[i].wait()) != hipSuccess) return e;  // its readers have finished
    c.dims[i][0] = 0;  // empty until the upload is enqueued
    uint64_t* h = reinterpret_cast<uint64_t*>(c.slot[i].host);
    uint8_t* d = c.slot[i].dev;
    if (!fill_bsr_addrs(h, a, base, ng, nw, rt, split)) return hipErrorInvalidValue;
    if ((e = hipMemcpyAsync(d, h, n * 8, hipMemcpyHostToDevice, stream)) != hipSuccess) return e;
    // (no event for the upload itself: the launch that follows on this stream records
    // the slot's event whether or not it is accepted, bsr_table_done, and that event
    // completes after the upload -- one hipEventRecord less in a first launch)
    std::memcpy(c.dims[i], dims, sizeof dims);
    c.coef[i] = m;
    *ref = BsrTblRef{&c, i, reinterpret_cast<const uint64_t*>(d)};
    return hipSuccess;
}

// Block pointers of a table-form launch into its arguments: false if k + r
// exceeds them.
bool bsr_tbl_ptrs(const ApplySpec& a, BsrTblJob& job) {
    if (size_t(a.k) + a.r > static_cast<size_t>(kBsrTblPtrs)) return false;
    for (uint32_t j = 0; j < a.k; ++j) job.ptr[j] = a.in[j];
    for (uint32_t i = 0; i < a.r; ++i) job.ptr[a.k + i] = a.out[i];
    return true;
}

// Waves (row tiles) per workgroup: one for r <= 10 (the one-wave form); 4 for
// r > 20 (tiles of <= 10 rows): 3 or 5 waves leave a SIMD of the CU with more
// of them than the others (one 64 MiB stripe: 20/50 0.062 ms with 3 tiles of
// 10 vs 0.056 with 4 of 8, 30/70 0.074 with 4 of 10 vs 0.091 with 5 of 8).
// 11-16 rows: 2 tiles of <= 8 (20/33: 0.031 ms, 4 tiles 0.035); 17-20 rows: 2
// tiles of 9-10 when the launch has units for >= 16 waves per CU (cfg4's
// 1024-stripe r = 20 decode: 0.469 ms, 3 tiles 0.475-0.48), else 4 tiles of 5
// (one 64 MiB 20/40 stripe: 0.044 ms, 2 tiles 0.053, 3 tiles 0.048).
// ZFEC_BSR_NW_WIDE: waves for r > 20 (default 4; the A/B knob of tools/ab_build.sh)
#ifndef ZFEC_BSR_NW_WIDE
#define ZFEC_BSR_NW_WIDE 4
#endif
void bsr_tiles(uint32_t r, uint64_t units, uint32_t* nw, uint32_t* rt) {
    if (r <= static_cast<uint32_t>(kBsrMaxRows))
        *nw = 1;
    else if (r <= 16 || (r <= 2u * kBsrMaxRows && units * 2 >= uint64_t(g_num_cu) * 16))
        *nw = 2;
    else
        *nw = ZFEC_BSR_NW_WIDE;
    *rt = (r + *nw - 1) / *nw;
}

bool bsr_shape_ok(uint32_t k, uint32_t r, uint64_t sz) {
    // kernel-argument form, or the table form past kBsrArgAddrs addresses
    return generic_mode() == 2 && k >= 1 && k <= static_cast<uint32_t>(kMaxIn) && r >= 1 &&
           r <= static_cast<uint32_t>(kBsrMaxOut) && sz >= kBsrChunk && k * r >= 24 && !(k <= 4 && r <= 8);
}

// Wide codes, one row tile: matapply_bsr_ks (table form).  Waves per unit:
// enough for ~8 waves per CU over the launch, 4-8, at least 4 inputs each.
constexpr uint32_t kBsrKsRows = 8;  // rows per group of the ks form past one tile
constexpr uint32_t kBsrTblTile = 8;

// The table form of the LDS-phase kernel (below) runs tiles of <= 8 rows in row
// groups of <= 8 tiles.  Round 4 used tiles of 4 for k > 64 in launches too
// small for 16 waves per CU; with the 8-wave groups sharing their inputs'
// combinations (bsr_cmb) a 4-row tile reads 30 LDS dwords per 4 rows and loses:
// 160/256 0.183 ms with tiles of 4 against 0.122 with 8 (profiles/r05_bsr_wide_ab.json).
//
// The ks form (inputs split over the waves of a workgroup) serves k > 32 with
// one row tile, and -- in row groups of 8, each re-reading the inputs -- launches
// of k >= 64 whose LDS-phase form would run fewer than 8 waves per CU (units x
// row groups x waves per group): 200/256 (164 units of 2 KiB per 64 MiB stripe,
// 1,312 waves) 0.082 ms on ks against 0.153, 96/128 (1,368 waves) 0.053 against
// 0.086; from there up the LDS-phase form wins: 160/256 (3,280 waves) 0.122,
// 64/112 (4,096) 0.070 -> 0.055, 128/256 0.121 (ks: 0.195 in round 4).
bool bsr_wide_ok(uint32_t k, uint32_t r, uint64_t sz, uint64_t nstripes) {
    if (generic_mode() != 2 || k <= static_cast<uint32_t>(kMaxIn) || k > static_cast<uint32_t>(kMaxWideIn) || r < 1 ||
        r > 256 || sz < kBsgChunk || k * r < 24)
        return false;
    if (r <= static_cast<uint32_t>(kBsrMaxRows)) return true;
    const uint64_t units = (sz + kBsrChunk - 1) / kBsrChunk * nstripes;
    const uint32_t ng = (r + 8 * kBsrTblTile - 1) / (8 * kBsrTblTile), rpg = (r + ng - 1) / ng;
    uint32_t nw = 1;  // as launch_bsr_tbl
    while (nw * kBsrTblTile < rpg) nw *= 2;
    return k >= 64 && units * ng * nw < uint64_t(g_num_cu) * 8;
}

struct BsrKsVariant {
    const void* fn = nullptr;
    KName name = "";
};
BsrKsVariant g_bsr_ks[kBsrMaxRows + 1];
std::once_flag g_bsr_ks_once;

void fill_bsr_ks() {
    for_each_rt<kBsrMaxRows>([](auto rt) {
        constexpr int RT = decltype(rt)::value;
        g_bsr_ks[RT].fn = reinterpret_cast<const void*>(matapply_bsr_ks<RT>);
        kname(g_bsr_ks[RT].name, "matapply_bsr", RT, ",ks,tbl");
    });
}

hipError_t launch_bsr_wide(const ApplySpec& a, hipStream_t stream) {
    std::call_once(g_bsr_ks_once, fill_bsr_ks);
    uint64_t base = 0;
    if (bsr_routine_base(&base, stream) != hipSuccess) return hipErrorNotSupported;
    const uint32_t k = a.k, r = a.r;
    const uint32_t ng = r <= static_cast<uint32_t>(kBsrMaxRows) ? 1u : (r + kBsrKsRows - 1) / kBsrKsRows;
    const uint32_t rt = (r + ng - 1) / ng;
    const uint64_t cps = (a.sz + kBsrChunk - 1) / kBsrChunk;
    const uint64_t units = cps * a.nstripes * ng;
    if (units >= (1ull << 32) - (1ull << 24)) return hipErrorInvalidValue;
    // waves per unit: 8 when the launch has fewer than 2 units per CU, else 4
    // (>= 4 inputs per wave); 16 waves measured slower on 94/100 (0.027 ->
    // 0.031 ms per 64 MiB stripe) and the same on 255/256
    uint32_t nw = units * 2 < uint64_t(g_num_cu) * 4 ? 8u : 4u;
    while (nw > 1 && k / nw < 4) nw /= 2;
    BsrTblJob job;
    if (!bsr_tbl_ptrs(a, job)) return hipErrorNotSupported;
    BsrTblRef t;
    hipError_t e = bsr_addr_table(a, stream, base, ng, 1, rt, nw, &t);
    if (e != hipSuccess) return e;
    const uint32_t grid = fill_units(job, a, cps, units, bsr_grid_cap());
    job.ngroups = ng;
    job.pad_ = 0;
    job.addr = t.dev;
    e = launch_job(g_bsr_ks[rt].fn, grid, 64 * nw, 0, stream, job);
    const hipError_t te = bsr_table_done(t, stream);  // also when the launch failed: the upload is a reader
    if (e != hipSuccess) return e;
    t_last_kernel = g_bsr_ks[rt].name;
    return te;
}

// Table form of the LDS-phase kernel: k > 32 with more than one row tile, or
// more rows than 4 tiles of 10.  Tiles of <= 8 rows (<= 127 VGPRs: 4 waves per
// SIMD), <= 8 waves per workgroup, so row groups of <= 64 rows; each group's
// workgroups read the unit's inputs again (L2 when they run together).
bool bsr_tbl_ok(uint32_t k, uint32_t r, uint64_t sz) {
    return generic_mode() == 2 && k >= 1 && k <= static_cast<uint32_t>(kMaxWideIn) && r >= 1 && r <= 256 &&
           sz >= kBsgChunk && k * r >= 24 && !(k <= 4 && r <= 8) &&
           (k > static_cast<uint32_t>(kMaxIn) ? r > static_cast<uint32_t>(kBsrMaxRows) : r > 4u * kBsrMaxRows);
}

struct BsrTblVariant {
    const void* fn = nullptr;
    const void* fn_cmb = nullptr;
    KName name = "";
    KName name_cmb = "";
};
BsrTblVariant g_bsr_tbl[kBsrMaxRows + 1];
std::once_flag g_bsr_tbl_once;

void fill_bsr_tbl() {
    for_each_rt<kBsrMaxRows>([](auto rt) {
        constexpr int RT = decltype(rt)::value;
        BsrTblVariant& v = g_bsr_tbl[RT];
        v.fn = reinterpret_cast<const void*>(matapply_bsr<RT, true, false, BsrTblJob>);
        v.fn_cmb = reinterpret_cast<const void*>(matapply_bsr<RT, true, true, BsrTblJob>);
        kname(v.name, "matapply_bsr", RT, ",lds,tbl");
        kname(v.name_cmb, "matapply_bsr", RT, ",lds,tbl,cmb");
    });
}

// One table-form launch of the LDS-phase kernel: ng row groups of nw waves of
// <= rt rows each.
hipError_t launch_bsr_lds_tbl(const ApplySpec& a, hipStream_t stream, uint64_t base, uint32_t ng, uint32_t nw,
                              uint32_t rt) {
    std::call_once(g_bsr_tbl_once, fill_bsr_tbl);
    const uint32_t k = a.k;
    const uint64_t cps = (a.sz + kBsrChunk - 1) / kBsrChunk;
    const uint64_t vunits = cps * a.nstripes * ng;
    if (vunits >= (1ull << 32) - (1ull << 24) || rt < 1 || rt > static_cast<uint32_t>(kBsrMaxRows))
        return hipErrorInvalidValue;
    BsrTblJob job;
    if (!bsr_tbl_ptrs(a, job)) return hipErrorNotSupported;
    BsrTblRef t;
    hipError_t e = bsr_addr_table(a, stream, base, ng, nw, rt, 1, &t);
    if (e != hipSuccess) return e;
    const uint32_t grid = fill_units(job, a, cps, vunits, bsr_grid_cap());
    job.ngroups = ng;
    job.pad_ = 0;
    job.addr = t.dev;
    const bool cmb = bsr_cmb(nw);
    e = launch_job(cmb ? g_bsr_tbl[rt].fn_cmb : g_bsr_tbl[rt].fn, grid, 64 * nw, bsr_lds_bytes(k, nw, cmb), stream, job);
    const hipError_t te = bsr_table_done(t, stream);  // also when the launch failed: the upload is a reader
    if (e != hipSuccess) return e;
    t_last_kernel = cmb ? g_bsr_tbl[rt].name_cmb : g_bsr_tbl[rt].name;
    return te;
}

hipError_t launch_bsr_tbl(const ApplySpec& a, hipStream_t stream) {
    uint64_t base = 0;
    if (bsr_routine_base(&base, stream) != hipSuccess) return hipErrorNotSupported;
    const uint32_t r = a.r, tile = kBsrTblTile;
    const uint32_t ng = (r + 8 * tile - 1) / (8 * tile);  // row groups of <= 8 waves
    const uint32_t rpg = (r + ng - 1) / ng;            // rows of the largest group
    uint32_t nw = 1;                                   // 1, 2, 4 or 8 waves: see bsr_tiles
    while (nw * tile < rpg) nw *= 2;
    return launch_bsr_lds_tbl(a, stream, base, ng, nw, (rpg + nw - 1) / nw);
}

hipError_t launch_bsr(const ApplySpec& a, hipStream_t stream) {
    std::call_once(g_bsr_once, fill_bsr);
    uint64_t base = 0;
    if (bsr_routine_base(&base, stream) != hipSuccess) return hipErrorNotSupported;
    const uint32_t k = a.k, r = a.r;
    const uint64_t cps = (a.sz + kBsrChunk - 1) / kBsrChunk;
    const uint64_t units = cps * a.nstripes;
    uint32_t nw, rt;
    bsr_tiles(r, units, &nw, &rt);
    if (units >= (1ull << 32) - (1ull << 24)) return hipErrorInvalidValue;
    // more addresses than the arguments hold (e.g. K=20/M=60's 40-row encode,
    // 800): the same kernel reading them from a device-side table
    if (size_t(nw) * k * rt > static_cast<size_t>(kBsrArgAddrs))
        return launch_bsr_lds_tbl(a, stream, base, 1, nw, rt);
    BsrJob job;
    const uint32_t grid = fill_units(job, a, cps, units, bsr_grid_cap());
    job.nt = nw;
    job.pad_ = 0;
    for (uint32_t j = 0; j < k; ++j) job.in[j] = a.in[j];
    for (uint32_t i = 0; i < r; ++i) job.out[i] = a.out[i];
    if (!fill_bsr_addrs(job.addr, a, base, 1, nw, rt, 1)) return hipErrorInvalidValue;
    if (nw == 1) {  // one row tile: one wave per unit, no LDS
        t_last_kernel = g_bsr_var[rt].name_solo;
        return launch_job(g_bsr_var[rt].fn_solo, grid, 64, 0, stream, job);
    }
    const bool cmb = bsr_cmb(nw);
    t_last_kernel = cmb ? g_bsr_var[rt].name_cmb : g_bsr_var[rt].name;
    return launch_job(cmb ? g_bsr_var[rt].fn_cmb : g_bsr_var[rt].fn, grid, 64 * nw, bsr_lds_bytes(k, nw, cmb), stream,
                      job);
}

// ---- matverify_bsr dispatch -------------------------------------------------------
// launch_bsr's choices for the same (k, r, units) -- the same tiles, the same
// walk order of the routine addresses, the same table cache -- with the verify
// kernels: one wave (r <= 10), the LDS-phase form with the addresses in the
// arguments, or in the device-side table past kBsrArgAddrs of them.
struct BsrVfyVariant {
    const void* fn_solo = nullptr;
    const void* fn = nullptr;
    const void* fn_tbl = nullptr;
    KName name_solo = "";
    KName name = "";
    KName name_tbl = "";
};
BsrVfyVariant g_bsr_vfy[kBsrMaxRows + 1];
std::once_flag g_bsr_vfy_once;

void fill_bsr_vfy() {
    for_each_rt<kBsrMaxRows>([](auto rt) {
        constexpr int RT = decltype(rt)::value;
        BsrVfyVariant& v = g_bsr_vfy[RT];
        v.fn_solo = reinterpret_cast<const void*>(matverify_bsr_solo<RT>);
        v.fn = reinterpret_cast<const void*>(matapply_bsr<RT, false, false, BsrVfyJob>);
        v.fn_tbl = reinterpret_cast<const void*>(matapply_bsr<RT, true, false, BsrVfyTblJob>);
        kname(v.name_solo, "matverify_bsr", RT, "");
        kname(v.name, "matverify_bsr", RT, ",lds");
        kname(v.name_tbl, "matverify_bsr", RT, ",lds,tbl");
    });
}

// The header every verify job shares, and the grid (launch_bsr's).
template <class J>
uint32_t bsr_vfy_header(J& job, const VerifySpec& v, uint64_t cps, uint64_t units) {
    job.sz = v.sz;
    job.in_sstride = v.sstride;
    job.mismatch = v.mismatch;
    job.nstripes = static_cast<uint32_t>(v.nstripes);
    job.k = v.k;
    job.r = v.r;
    job.words = v.words;
    job.bit0 = v.bit0;
    return fill_stride(job, cps, units, bsr_grid_cap());
}

hipError_t launch_verify_bsr_one(const VerifySpec& v, hipStream_t stream) {
    std::call_once(g_bsr_vfy_once, fill_bsr_vfy);
    uint64_t base = 0;
    if (bsr_routine_base(&base, stream) != hipSuccess) return hipErrorNotSupported;
    const uint32_t k = v.k, r = v.r;
    const uint64_t cps = (v.sz + kBsrChunk - 1) / kBsrChunk;
    const uint64_t units = cps * v.nstripes;
    if (units >= (1ull << 32) - (1ull << 24)) return hipErrorNotSupported;
    uint32_t nw, rt;
    bsr_tiles(r, units, &nw, &rt);
    ApplySpec a{};  // what fill_bsr_addrs and the table cache read: the matrix
    a.coef = v.coef;
    a.coef_stride = v.coef_stride;
    a.k = k;
    a.r = r;
    if (size_t(nw) * k * rt > static_cast<size_t>(kBsrArgAddrs)) {
        if (nw == 1 || k + r > static_cast<uint32_t>(kBsrVfyPtrs)) return hipErrorNotSupported;
        BsrVfyTblJob job;
        BsrTblRef t;
        hipError_t e = bsr_addr_table(a, stream, base, 1, nw, rt, 1, &t);
        if (e != hipSuccess) return e == hipErrorInvalidValue ? hipErrorNotSupported : e;
        const uint32_t grid = bsr_vfy_header(job, v, cps, units);
        job.ngroups = 1;
        job.pad_ = 0;
        job.addr = t.dev;
        for (uint32_t j = 0; j < k; ++j) job.ptr[j] = v.in[j];
        for (uint32_t i = 0; i < r; ++i) job.ptr[k + i] = v.chk[i];
        e = launch_job(g_bsr_vfy[rt].fn_tbl, grid, 64 * nw, bsr_lds_bytes(k, nw, false), stream, job);
        const hipError_t te = bsr_table_done(t, stream);  // also when the launch failed: the upload is a reader
        if (e != hipSuccess) return e;
        t_last_kernel = g_bsr_vfy[rt].name_tbl;
        return te;
    }
    BsrVfyJob job;
    const uint32_t grid = bsr_vfy_header(job, v, cps, units);
    for (uint32_t j = 0; j < k; ++j) job.in[j] = v.in[j];
    for (uint32_t i = 0; i < r; ++i) job.out[i] = v.chk[i];
    if (!fill_bsr_addrs(job.addr, a, base, 1, nw, rt, 1)) return hipErrorNotSupported;
    const hipError_t e = nw == 1 ? launch_job(g_bsr_vfy[rt].fn_solo, grid, 64, 0, stream, job)
                                 : launch_job(g_bsr_vfy[rt].fn, grid, 64 * nw, bsr_lds_bytes(k, nw, false), stream, job);
    if (e == hipSuccess) t_last_kernel = nw == 1 ? g_bsr_vfy[rt].name_solo : g_bsr_vfy[rt].name;
    return e;
}

// ---- matapply_mixed dispatch ------------------------------------------------------
// Staging of a mixed call's pattern tables and host-side ids, per thread and
// device.  The TableRing pattern -- a pinned host slot, its device twin filled
// by one stream-ordered copy, an event recorded after the slot's last launch
// and waited for before the slot is rewritten, so consecutive calls (on any
// streams) never share a slot in flight -- with slots that grow to what a call
// needs: 4096 K=4 patterns are 1.3 MB of tables, 10^6 host-side ids 4 MB.
struct MixedRing {
    static constexpr int kSlots = 4;
    Slot slot[kSlots];
    size_t cap[kSlots] = {};
    unsigned next = 0;
    void release() {
        for (Slot& s : slot) s.drop_event(), s.free_mem();
    }
};
thread_local PerDevice<MixedRing> t_mixed_rings;

hipError_t mixed_slot(size_t bytes, Slot** out) {
    MixedRing* t = nullptr;
    hipError_t e = t_mixed_rings.here(&t);
    if (e != hipSuccess) return e;
    const unsigned i = t->next++ % MixedRing::kSlots;
    Slot& s = t->slot[i];
    if ((e = s.event()) != hipSuccess || (e = s.wait()) != hipSuccess) return e;  // its last launch has read it
    if (t->cap[i] < bytes) {
        s.free_mem();
        t->cap[i] = 0;
        const size_t cap = (std::max<size_t>(bytes, size_t(64) << 10) + 4095) / 4096 * 4096;
        if ((e = s.alloc(cap)) != hipSuccess) return e;
        t->cap[i] = cap;
    }
    *out = &s;
    return hipSuccess;
}

// One stream-ordered upload through a MixedRing slot: acquire(), fill host(),
// copy(), launch what reads dev(), then done() -- also after a failed launch,
// since the copy reads the slot whatever happened.
struct StagedUpload {
    Slot* slot = nullptr;
    hipError_t acquire(size_t bytes) { return mixed_slot(bytes, &slot); }
    uint8_t* host() const { return slot->host; }
    const uint8_t* dev() const { return slot->dev; }
    hipError_t copy(size_t bytes, hipStream_t stream) const {
        return hipMemcpyAsync(slot->dev, slot->host, bytes, hipMemcpyHostToDevice, stream);
    }
    void done(hipStream_t stream) const {
        if (slot->record(stream) != hipSuccess) (void)hipStreamSynchronize(stream);
    }
};

// The wave-inside-one-stripe walk (WaveWalk) of a launch over ns stripes of
// len bytes, by workgroups of wg_waves waves, at most `cap` of them; returns
// the grid.
uint32_t fill_walk(Walk& k, uint64_t len, uint64_t ns, uint64_t wg_waves, uint64_t cap) {
    const uint64_t cps = (len + kChunk - 1) / kChunk, wps = (cps + 63) / 64;
    const uint64_t waves = ns * wps, need = (waves + wg_waves - 1) / wg_waves;
    const uint32_t grid = static_cast<uint32_t>(need < cap ? need : cap);
    const uint64_t gstride = uint64_t(grid) * wg_waves;
    k.sz = len;
    k.nstripes = static_cast<uint32_t>(ns);
    k.cps = static_cast<uint32_t>(cps);
    k.wps = static_cast<uint32_t>(wps);
    k.gs_s = static_cast<uint32_t>(gstride / wps);
    k.gs_w = static_cast<uint32_t>(gstride % wps);
    k.pad_ = 0;
    return grid;
}
uint32_t fill_walk(Walk& k, uint64_t len, uint64_t ns) { return fill_walk(k, len, ns, kBlock / 64, unit_grid_cap()); }

// Launches of at most Config::launch_units lanes: blocks longer than that many
// 16-byte chunks are cut into byte ranges (whole waves of 1 KiB), batches into
// stripe groups.  f(b0, len, s0, ns) makes one launch.
template <class F>
hipError_t launch_pieces(uint64_t sz, uint64_t nstripes, F&& f) {
    const uint64_t max_units = config().launch_units;
    const uint64_t piece = (max_units & ~uint64_t(63)) * kChunk;
    for (uint64_t b0 = 0; b0 < sz; b0 += piece) {
        const uint64_t len = std::min(piece, sz - b0);
        const uint64_t wps = ((len + kChunk - 1) / kChunk + 63) / 64;
        const uint64_t group = std::max<uint64_t>(1, max_units / (wps * 64));
        for (uint64_t s0 = 0; s0 < nstripes; s0 += group) {
            const hipError_t e = f(b0, len, s0, std::min(group, nstripes - s0));
            if (e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

template <int K>
hipError_t launch_mixed_k(const MixedSpec& m, hipStream_t stream) {
    static const char* const kNames[kMixedMaxK + 1] = {"", "matapply_mixed<1>", "matapply_mixed<2>",
                                                       "matapply_mixed<3>", "matapply_mixed<4>"};
    constexpr uint32_t TD = mixed_tab_dwords<K>();
    const size_t tab_bytes = (size_t(m.npatterns) * TD * 4 + 255) / 256 * 256;
    const size_t ids_bytes = m.ids_host ? size_t(m.nstripes) * 4 : 0;
    StagedUpload up;
    hipError_t e = up.acquire(tab_bytes + ids_bytes);
    if (e != hipSuccess) return e;
    uint32_t* ht = reinterpret_cast<uint32_t*>(up.host());
    for (size_t p = 0; p < m.npatterns; ++p) {
        uint32_t* t = ht + p * TD;
        for (int i = 0; i < K * K; ++i) host_tab(t + i * 5, m.rows[p * K * K + i]);
        for (uint32_t i = K * K * 5; i < TD; ++i) t[i] = 0;
    }
    if (ids_bytes) std::memcpy(up.host() + tab_bytes, m.ids_host, ids_bytes);
    if ((e = up.copy(tab_bytes + ids_bytes, stream)) != hipSuccess) return e;
    const uint32_t* ids = m.ids_host ? reinterpret_cast<const uint32_t*>(up.dev() + tab_bytes) : m.ids_dev;
    MixedJob<K> job;
    job.in_sstride = m.in_sstride;
    job.out_sstride = m.out_sstride;
    job.npatterns = m.npatterns;
    job.tables = reinterpret_cast<const uint32_t*>(up.dev());
    // the id pointer advances per stripe group
    e = launch_pieces(m.sz, m.nstripes, [&](uint64_t b0, uint64_t len, uint64_t s0, uint64_t ns) {
        const uint32_t grid = fill_walk(job.walk, len, ns);
        job.ids = ids + s0;
        for (int j = 0; j < K; ++j) {
            job.in[j] = m.in[j] + b0 + s0 * m.in_sstride;
            job.out[j] = m.out[j] + b0 + s0 * m.out_sstride;
        }
        return launch_job(reinterpret_cast<const void*>(matapply_mixed<K>), grid, kBlock, 0, stream, job);
    });
    up.done(stream);
    if (e == hipSuccess) t_last_kernel = kNames[K];
    return e;
}

// ---- parity verification dispatch (matverify_reg, rows_differ) ---------------------
// The three <K, R> families (matverify_reg, matlocate_reg, matrepair_mixed):
// name[k][r] = "kernel<k,r>", and table(k, r) = L::launch<k, r> for 1 <= k <=
// kRegK, RMin <= r <= kRegR (null at k = 0 and below RMin).
struct KrNames {
    char name[kRegK + 1][kRegR + 1][28];
    explicit KrNames(const char* kernel) {
        for (int k = 1; k <= kRegK; ++k)
            for (int r = 1; r <= kRegR; ++r) snprintf(name[k][r], sizeof name[k][r], "%s<%d,%d>", kernel, k, r);
    }
};

template <class L, int RMin = 1>
struct KrTable {
    typedef decltype(&L::template launch<1, RMin>) Fn;
    template <int K, int R>
    static constexpr Fn pick() {
        if constexpr (K >= 1 && R >= RMin)
            return &L::template launch<K, R>;
        else
            return nullptr;
    }
    template <int... I>
    static constexpr std::array<Fn, sizeof...(I)> all(std::integer_sequence<int, I...>) {
        return {{pick<I / (kRegR + 1), I % (kRegR + 1)>()...}};
    }
    std::array<Fn, (kRegK + 1) * (kRegR + 1)> fn = all(std::make_integer_sequence<int, (kRegK + 1) * (kRegR + 1)>());
    constexpr Fn operator()(uint32_t k, uint32_t r) const { return fn[k * (kRegR + 1) + r]; }
};

// The r x k tables of `v.coef` in the RegJob layout.
template <int K, int R>
void fill_tabs(uint32_t* tab, const VerifySpec& v) {
    for (int i = 0; i < R; ++i)
        for (int j = 0; j < K; ++j) host_tab(&tab[(i * K + j) * 5], v.coef[size_t(i) * v.coef_stride + j]);
}

struct LocateArgs {
    const uint8_t* q;  // (r-1) x k
    uint32_t xbit;
};

const KrNames g_verify_names("matverify_reg"), g_locate_names("matlocate_reg");

// matverify_reg<K, R> or matlocate_reg<K, R> (a: the locate call's Q and xbit).
template <int K, int R, bool LOC>
hipError_t launch_scrub(const VerifySpec& v, const LocateArgs* a, hipStream_t stream) {
    ScrubJob<K, R, LOC> job;
    job.sstride = v.sstride;
    job.words = v.words;
    job.bit0 = v.bit0;
    job.xbit = 0;
    job.qtab[0] = 0;
    fill_tabs<K, R>(job.tab, v);
    if constexpr (LOC) {
        job.xbit = a->xbit;
        for (int i = 0; i < (R - 1) * K; ++i) host_tab(&job.qtab[i * 5], a->q[i]);
    }
    const void* fn;
    if constexpr (LOC)
        fn = reinterpret_cast<const void*>(matlocate_reg<K, R>);
    else
        fn = reinterpret_cast<const void*>(matverify_reg<K, R>);
    const hipError_t e = launch_pieces(v.sz, v.nstripes, [&](uint64_t b0, uint64_t len, uint64_t s0, uint64_t ns) {
        const uint32_t grid = fill_walk(job.walk, len, ns);
        job.bits = v.mismatch + s0 * v.words;
        for (int j = 0; j < K; ++j) job.in[j] = v.in[j] + b0 + s0 * v.sstride;
        for (int i = 0; i < R; ++i) job.chk[i] = v.chk[i] + b0 + s0 * v.sstride;
        return launch_job(fn, grid, kBlock, 0, stream, job);
    });
    if (e == hipSuccess) t_last_kernel = (LOC ? g_locate_names : g_verify_names).name[K][R];
    return e;
}

struct VerifyKr {
    template <int K, int R>
    static hipError_t launch(const VerifySpec& v, hipStream_t stream) {
        return launch_scrub<K, R, false>(v, nullptr, stream);
    }
};
constexpr KrTable<VerifyKr> g_verify_launch;

// ---- error location dispatch (matlocate_reg) ------------------------------------------
struct LocateKr {
    template <int K, int R>
    static hipError_t launch(const VerifySpec& v, const LocateArgs& a, hipStream_t stream) {
        return launch_scrub<K, R, true>(v, &a, stream);
    }
};
constexpr KrTable<LocateKr, 2> g_locate_launch;

// ---- matrepair_mixed dispatch ------------------------------------------------------
// One upload through a MixedRing slot (the records, then any host-side ids)
// serves every row group of a call.
struct RepairUpload {
    const uint32_t* records;  // device
    const uint32_t* ids;      // device
    uint32_t rec_dwords, mask_off;
};

constexpr uint32_t repair_rec_dwords(uint32_t k, uint32_t t) { return (t * k * 5 + 1 + 3) / 4 * 4; }

const KrNames g_repair_names("matrepair_mixed");

// Rows [g0, g0 + R) of every stripe.
struct RepairKr {
    template <int K, int R>
    static hipError_t launch(const RepairSpec& p, const RepairUpload& u, uint32_t g0, hipStream_t stream) {
        RepairJob<K, R> job;
        job.in_sstride = p.in_sstride;
        job.out_sstride = p.out_sstride;
        job.npatterns = p.npatterns;
        job.rec_dwords = u.rec_dwords;
        job.tab_off = g0 * K * 5;
        job.mask_off = u.mask_off;
        job.bit0 = g0;
        job.records = u.records;
        const hipError_t e = launch_pieces(p.sz, p.nstripes, [&](uint64_t b0, uint64_t len, uint64_t s0, uint64_t ns) {
            const uint32_t grid = fill_walk(job.walk, len, ns);
            job.ids = u.ids + s0;
            for (int j = 0; j < K; ++j) job.in[j] = p.in[j] + b0 + s0 * p.in_sstride;
            for (int i = 0; i < R; ++i) job.out[i] = p.out[g0 + i] + b0 + s0 * p.out_sstride;
            return launch_job(reinterpret_cast<const void*>(matrepair_mixed<K, R>), grid, kBlock, 0, stream, job);
        });
        if (e == hipSuccess) t_last_kernel = g_repair_names.name[K][R];
        return e;
    }
};
constexpr KrTable<RepairKr> g_repair_launch;

// The live rows of all patterns together.
uint32_t repair_any(const uint32_t* masks, size_t npatterns, uint32_t t) {
    uint32_t any = 0;
    for (size_t q = 0; q < npatterns; ++q) any |= masks[q];
    return t < 32 ? any & ((1u << t) - 1u) : any;
}

// Build records: npatterns matrepair_mixed records into host memory.
void repair_fill_records(uint32_t* ht, const uint8_t* rows, const uint32_t* masks, size_t npatterns, uint32_t k,
                         uint32_t t) {
    const uint32_t rec_dwords = repair_rec_dwords(k, t), mask_off = t * k * 5;
    for (size_t q = 0; q < npatterns; ++q) {
        uint32_t* rec = ht + q * rec_dwords;
        for (uint32_t i = 0; i < t * k; ++i) host_tab(rec + i * 5, rows[q * t * k + i]);
        rec[mask_off] = masks[q];
        for (uint32_t i = mask_off + 1; i < rec_dwords; ++i) rec[i] = 0;
    }
}

// Launch over records: the row groups of 8 that some pattern stores (`any`),
// records and ids in device memory.
hipError_t launch_repair_groups(const RepairSpec& p, const uint32_t* records, const uint32_t* ids, uint32_t any,
                                hipStream_t stream) {
    const uint32_t k = p.k, t = p.t;
    RepairUpload u;
    u.rec_dwords = repair_rec_dwords(k, t);
    u.mask_off = t * k * 5;
    u.records = records;
    u.ids = ids;
    hipError_t e = hipSuccess;
    for (uint32_t g0 = 0; g0 < t && e == hipSuccess; g0 += kRegR) {
        const uint32_t rg = std::min<uint32_t>(kRegR, t - g0);
        if (!((any >> g0) & ((1u << rg) - 1u))) continue;  // rows no pattern stores
        e = g_repair_launch(k, rg)(p, u, g0, stream);
    }
    return e;
}

hipError_t launch_repair_all(const RepairSpec& p, hipStream_t stream) {
    const uint32_t k = p.k, t = p.t;
    const uint32_t any = repair_any(p.masks, p.npatterns, t);
    if (!any) return hipSuccess;  // nothing to store: no upload, no launch
    const size_t tab_bytes = (size_t(p.npatterns) * repair_rec_dwords(k, t) * 4 + 255) / 256 * 256;
    const size_t ids_bytes = p.ids_host ? size_t(p.nstripes) * 4 : 0;
    StagedUpload up;
    hipError_t e = up.acquire(tab_bytes + ids_bytes);
    if (e != hipSuccess) return e;
    repair_fill_records(reinterpret_cast<uint32_t*>(up.host()), p.rows, p.masks, p.npatterns, k, t);
    if (ids_bytes) std::memcpy(up.host() + tab_bytes, p.ids_host, ids_bytes);
    if ((e = up.copy(tab_bytes + ids_bytes, stream)) != hipSuccess) return e;
    e = launch_repair_groups(p, reinterpret_cast<const uint32_t*>(up.dev()),
                             p.ids_host ? reinterpret_cast<const uint32_t*>(up.dev() + tab_bytes) : p.ids_dev, any,
                             stream);
    up.done(stream);
    return e;
}

// ---- matupdate_reg dispatch ----------------------------------------------------------
// One upload through a MixedRing slot (the k records, then any host-side
// numbers) serves every row group of a call.
struct UpdateUpload {
    const uint32_t* records;  // device
    const uint32_t* changed;  // device
    uint32_t rec_dwords, mask_off;
};

constexpr uint32_t update_rec_dwords(uint32_t nrows) { return (nrows * 5 + (nrows + 31) / 32 + 3) / 4 * 4; }

// The k records of an update at `ht`: record j the tables of coefs[j * nrows + i]
// for every row i, then the live-row mask dwords, padded to 16 bytes.
void update_fill_records(uint32_t* ht, const uint8_t* coefs, uint32_t k, uint32_t nrows) {
    const uint32_t rec_dwords = update_rec_dwords(nrows), mask_off = nrows * 5;
    for (uint32_t j = 0; j < k; ++j) {
        uint32_t* rec = ht + size_t(j) * rec_dwords;
        for (uint32_t i = mask_off; i < rec_dwords; ++i) rec[i] = 0;
        for (uint32_t i = 0; i < nrows; ++i) {
            const uint8_t coef = coefs[size_t(j) * nrows + i];
            host_tab(rec + i * 5, coef);
            if (coef) rec[mask_off + i / 32] |= 1u << (i % 32);
        }
    }
}

const KrNames g_update_names("matupdate_reg");

// Rows [g0, g0 + R) of every stripe; K is the number of input slots.
struct UpdateKr {
    template <int K, int R>
    static hipError_t launch(const UpdateSpec& p, const UpdateUpload& u, uint32_t g0, hipStream_t stream) {
        UpdateJob<K, R> job;
        job.in_sstride = p.in_sstride;
        job.row_sstride = p.row_sstride;
        job.k = p.k;
        job.rec_dwords = u.rec_dwords;
        job.tab_off = g0 * 5;
        job.mask_off = u.mask_off + g0 / 32;
        job.bit0 = g0 % 32;
        job.has_old = p.oldb != nullptr;
        job.records = u.records;
        const hipError_t e = launch_pieces(p.sz, p.nstripes, [&](uint64_t b0, uint64_t len, uint64_t s0, uint64_t ns) {
            const uint32_t grid = fill_walk(job.walk, len, ns);
            job.changed = u.changed + s0 * K;
            for (int c = 0; c < K; ++c) {
                const uint64_t off = b0 + s0 * p.in_sstride + c * p.in_bstride;
                job.nw[c] = p.newb + off;
                job.od[c] = p.oldb ? p.oldb + off : nullptr;
            }
            for (int i = 0; i < R; ++i) job.row[i] = p.rows[g0 + i] + b0 + s0 * p.row_sstride;
            return launch_job(reinterpret_cast<const void*>(matupdate_reg<K, R>), grid, kBlock, 0, stream, job);
        });
        if (e == hipSuccess) t_last_kernel = g_update_names.name[K][R];
        return e;
    }
};
constexpr KrTable<UpdateKr> g_update_launch;

hipError_t launch_update_all(const UpdateSpec& p, hipStream_t stream) {
    const uint32_t rec_dwords = update_rec_dwords(p.nrows), mask_off = p.nrows * 5;
    const size_t tab_bytes = (size_t(p.k) * rec_dwords * 4 + 255) / 256 * 256;
    const size_t ch_bytes = p.changed_host ? size_t(p.nstripes) * p.c * 4 : 0;
    StagedUpload up;
    hipError_t e = up.acquire(tab_bytes + ch_bytes);
    if (e != hipSuccess) return e;
    update_fill_records(reinterpret_cast<uint32_t*>(up.host()), p.coefs, p.k, p.nrows);
    if (ch_bytes) std::memcpy(up.host() + tab_bytes, p.changed_host, ch_bytes);
    if ((e = up.copy(tab_bytes + ch_bytes, stream)) != hipSuccess) return e;
    UpdateUpload u;
    u.records = reinterpret_cast<const uint32_t*>(up.dev());
    u.changed = p.changed_host ? reinterpret_cast<const uint32_t*>(up.dev() + tab_bytes) : p.changed_dev;
    u.rec_dwords = rec_dwords;
    u.mask_off = mask_off;
    for (uint32_t g0 = 0; g0 < p.nrows && e == hipSuccess; g0 += kRegR)
        e = g_update_launch(p.c, std::min<uint32_t>(kRegR, p.nrows - g0))(p, u, g0, stream);
    up.done(stream);
    return e;
}

// ---- matapply_ragged dispatch ---------------------------------------------------------
// The grid of matapply_ragged: a wave per unit where a unit moves 10 KiB or more
// (k + r >= 10: the K=3/M=10 encode), else the fewest units per wave that do --
// two for that code's two-row decode.  Measured on 10^6 stripes of 4 KiB against
// the uniform call (profiles/ragged_bench.json): the
// encode 0.96 x with one unit per wave, 1.00 with two, 1.02 with four and 1.05
// with 122 (a grid of 32 workgroups per CU); the decode 1.25 x with one, 0.95
// with two, 1.02 with four.  Short ranges keep neighbouring waves on
// neighbouring KiBs, as the grid-stride walk of the other kernels does; a wave
// that moves too little cannot hide its one search over ustart.  The cap is the
// unit kernels' (CUs x 8192 workgroups); past it the ranges lengthen.
constexpr uint64_t kRaggedGridPerCu = kGridPerCu;
constexpr uint32_t kRaggedWaveKiB = 10;
constexpr uint64_t ragged_units_per_wave(uint32_t k, uint32_t r) { return (kRaggedWaveKiB + k + r - 1) / (k + r); }

// grid = min(ceil(units / (per_wave * waves per workgroup)), cap)
uint32_t ragged_grid(uint64_t units, uint64_t per_wave) {
    const uint64_t cap = hooked_grid_cap(uint64_t(g_num_cu) * kRaggedGridPerCu);
    const uint64_t per_wg = per_wave * (kBlock / 64), need = (units + per_wg - 1) / per_wg;
    return static_cast<uint32_t>(need < cap ? need : cap);
}

// What a ragged call staged, in device memory: the descriptor arrays (one or
// two offset arrays) and the call's own head bytes (a repair's records and ids).
struct RaggedDev {
    const uint64_t *ustart, *sizes, *off[2];
    const uint8_t* head;
};

const KrNames g_ragged_names("matapply_ragged");

// Rows [g0, g0 + R) of every stripe.
struct RaggedKr {
    template <int K, int R>
    static hipError_t launch(const RaggedSpec& p, const RaggedDev& d, uint32_t g0, uint32_t grid,
                             hipStream_t stream) {
        RaggedJob<K, R> job;
        job.in_bstride = p.in_bstride;
        job.out_bstride = p.out_bstride;
        job.in_bytes = p.in_bytes;
        job.out_bytes = p.out_bytes;
        job.nstripes = static_cast<uint32_t>(p.nstripes);
        job.rows_all = p.r;
        job.row0 = g0;
        job.pad_ = 0;
        job.ustart = d.ustart;
        job.sizes = d.sizes;
        job.in_off = d.off[0];
        job.out_off = d.off[1];
        job.in = p.in;
        job.out = p.out;
        for (int i = 0; i < R * K; ++i) host_tab(&job.tab[i * 5], p.coef[size_t(g0) * K + i]);
        const hipError_t e =
            launch_job(reinterpret_cast<const void*>(matapply_ragged<K, R>), grid, kBlock, 0, stream, job);
        if (e == hipSuccess) t_last_kernel = g_ragged_names.name[K][R];
        return e;
    }
};
constexpr KrTable<RaggedKr> g_ragged_launch;

// ustart of device-side sizes into `ustart` (n + 1 words) with `tsum` (one word
// per tile) as scratch, both device memory: the three phases of ragged_scan.
hipError_t launch_ragged_scan(const uint64_t* sizes, uint64_t n, uint64_t maxsz, uint64_t* ustart, uint64_t* tsum,
                              hipStream_t stream) {
    ScanJob job;
    job.sizes = sizes;
    job.ustart = ustart;
    job.tsum = tsum;
    job.n = n;
    job.maxsz = maxsz;
    job.ntiles = static_cast<uint32_t>((n + kScanTile - 1) / kScanTile);
    job.pad_ = 0;
    hipError_t e = launch_job(reinterpret_cast<const void*>(ragged_scan<0>), job.ntiles, kBlock, 0, stream, job);
    if (e == hipSuccess) e = launch_job(reinterpret_cast<const void*>(ragged_scan<1>), 1, kBlock, 0, stream, job);
    if (e == hipSuccess)
        e = launch_job(reinterpret_cast<const void*>(ragged_scan<2>), job.ntiles, kBlock, 0, stream, job);
    return e;
}

// The descriptor staging of a ragged call through one MixedRing slot, after
// `head` bytes of the call's own (fill_head(host address) writes them; a
// multiple of 256).  Host-side arrays: [head | ustart | sizes | off...] by one
// copy.  Device-side arrays: the head by one copy, ragged_scan's ustart (sizes
// past scan_maxsz counting no units) and its tile sums behind it in the slot's
// device half, sizes and offsets where the caller has them.  `units`
// afterwards: the call's total, 0 when every stripe is empty (nothing was
// copied: the caller returns, nothing to launch); with device-side arrays
// `estimate`, which only sizes the grid.  On success with units != 0 the
// caller launches what reads `d` and the head at up.dev(), then up.done() --
// also after a failed launch; after an error here there is nothing to undo.
//
// The estimate: blocks do not overlap, so the sizes sum to at most an arena
// over its rows (ragged_units_bound).  The rounding of each stripe's last unit
// is left out: a total above the estimate lengthens the ranges a little, one
// below it leaves waves with less than their share (or nothing: they exit),
// which is what a narrow shape cannot afford (ragged_units_per_wave).
uint64_t ragged_units_bound(uint64_t bytes, uint64_t bstride, uint32_t rows) {
    return bytes / (bstride ? 1 : rows) / kRaggedUnit;
}

struct RaggedStage {
    StagedUpload up;
    RaggedDev d{};
    uint64_t units = 0;

    template <class Fill>
    hipError_t stage(const uint64_t* sizes, std::initializer_list<const uint64_t*> offs, uint64_t ns, bool desc_host,
                     uint64_t scan_maxsz, uint64_t estimate, size_t head, Fill fill_head, hipStream_t stream) {
        const uint64_t ntiles = (ns + kScanTile - 1) / kScanTile;
        const size_t bytes = head + ((desc_host ? (1 + offs.size()) * ns : ntiles) + ns + 1) * sizeof(uint64_t);
        hipError_t e = up.acquire(bytes);
        if (e != hipSuccess) return e;
        d.head = up.dev();
        if (desc_host) {
            uint64_t* const h = reinterpret_cast<uint64_t*>(up.host() + head);
            if (!(units = ragged_units(sizes, ns, h))) return hipSuccess;
            fill_head(up.host());
            const uint64_t* const dv = reinterpret_cast<const uint64_t*>(up.dev() + head);
            size_t at = ns + 1;
            std::memcpy(h + at, sizes, ns * sizeof(uint64_t));
            d.ustart = dv;
            d.sizes = dv + at;
            int i = 0;
            for (const uint64_t* o : offs) {
                at += ns;
                std::memcpy(h + at, o, ns * sizeof(uint64_t));
                d.off[i++] = dv + at;
            }
            return up.copy(bytes, stream);
        }
        units = std::max<uint64_t>(1, estimate);
        if (head) {
            fill_head(up.host());
            if ((e = up.copy(head, stream)) != hipSuccess) return e;
        }
        uint64_t* const dv = reinterpret_cast<uint64_t*>(up.slot->dev + head);
        if ((e = launch_ragged_scan(sizes, ns, scan_maxsz, dv, dv + ns + 1, stream)) != hipSuccess) {
            up.done(stream);
            return e;
        }
        d.ustart = dv;
        d.sizes = sizes;
        int i = 0;
        for (const uint64_t* o : offs) d.off[i++] = o;
        return hipSuccess;
    }
};

hipError_t launch_ragged_all(const RaggedSpec& p, hipStream_t stream) {
    RaggedStage st;
    hipError_t e = st.stage(p.sizes, {p.in_off, p.out_off}, p.nstripes, p.desc_host, std::min(p.in_bytes, p.out_bytes),
                            std::min(ragged_units_bound(p.in_bytes, p.in_bstride, p.k),
                                     ragged_units_bound(p.out_bytes, p.out_bstride, p.r)),
                            0, [](uint8_t*) {}, stream);
    if (e != hipSuccess || !st.units) return e;
    for (uint32_t g0 = 0; g0 < p.r && e == hipSuccess; g0 += kRegR) {
        const uint32_t rg = std::min<uint32_t>(kRegR, p.r - g0);
        e = g_ragged_launch(p.k, rg)(p, st.d, g0, ragged_grid(st.units, ragged_units_per_wave(p.k, rg)), stream);
    }
    st.up.done(stream);
    return e;
}

// ---- matverify_ragged / matlocate_ragged dispatch -------------------------------------
const KrNames g_ragged_verify_names("matverify_ragged");
const KrNames g_ragged_locate_names("matlocate_ragged");

template <int K, int R, bool LOC>
hipError_t launch_ragged_scrub_kr(const RaggedScrubSpec& p, const RaggedDev& d, uint32_t g0, uint32_t grid,
                                  hipStream_t stream) {
    RaggedScrubJob<K, R, LOC> job;
    job.bstride = p.bstride;
    job.bytes = p.bytes;
    job.nstripes = static_cast<uint32_t>(p.nstripes);
    job.slots = p.k + p.c;
    job.chk0 = p.k + g0;
    job.bit0 = g0;
    job.words = p.words;
    job.xbit = p.xbit;
    job.ustart = d.ustart;
    job.sizes = d.sizes;
    job.off = d.off[0];
    job.src = p.src;
    job.bits = p.bits;
    for (int i = 0; i < R * K; ++i) host_tab(&job.tab[i * 5], p.P[size_t(g0) * K + i]);
    job.qtab[0] = 0;
    if constexpr (LOC)
        for (int i = 0; i < (R - 1) * K; ++i) host_tab(&job.qtab[i * 5], p.Q[i]);
    const void* fn;
    if constexpr (LOC)
        fn = reinterpret_cast<const void*>(matlocate_ragged<K, R>);
    else
        fn = reinterpret_cast<const void*>(matverify_ragged<K, R>);
    const hipError_t e = launch_job(fn, grid, kBlock, 0, stream, job);
    if (e == hipSuccess) t_last_kernel = (LOC ? g_ragged_locate_names : g_ragged_verify_names).name[K][R];
    return e;
}

struct RaggedVerifyKr {
    template <int K, int R>
    static hipError_t launch(const RaggedScrubSpec& p, const RaggedDev& d, uint32_t g0, uint32_t grid,
                             hipStream_t stream) {
        return launch_ragged_scrub_kr<K, R, false>(p, d, g0, grid, stream);
    }
};
struct RaggedLocateKr {
    template <int K, int R>
    static hipError_t launch(const RaggedScrubSpec& p, const RaggedDev& d, uint32_t g0, uint32_t grid,
                             hipStream_t stream) {
        return launch_ragged_scrub_kr<K, R, true>(p, d, g0, grid, stream);
    }
};
constexpr KrTable<RaggedVerifyKr> g_ragged_verify_launch;
constexpr KrTable<RaggedLocateKr, 2> g_ragged_locate_launch;

// The grid rule is matapply_ragged's, ceil(10 / (k + r)) units per wave with r
// the launch's checks: measured there for stored rows at k + r = 10 and 5, not
// for this read-only traffic.
hipError_t launch_ragged_scrub_all(const RaggedScrubSpec& p, hipStream_t stream) {
    RaggedStage st;
    hipError_t e = st.stage(p.sizes, {p.off}, p.nstripes, p.desc_host, p.bytes,
                            ragged_units_bound(p.bytes, p.bstride, p.k + p.c), 0, [](uint8_t*) {}, stream);
    if (e != hipSuccess || !st.units) return e;
    for (uint32_t g0 = 0; g0 < p.c && e == hipSuccess; g0 += kRegR) {
        const uint32_t rg = std::min<uint32_t>(kRegR, p.c - g0);
        const uint32_t grid = ragged_grid(st.units, ragged_units_per_wave(p.k, rg));
        e = p.Q ? g_ragged_locate_launch(p.k, rg)(p, st.d, g0, grid, stream)
                : g_ragged_verify_launch(p.k, rg)(p, st.d, g0, grid, stream);
    }
    if (p.keep && e == hipSuccess) {
        // a correction follows over the same descriptors: it releases the slot (ragged_scrub_release)
        *p.keep = RaggedScrubStaged{st.up.slot, st.d.ustart, st.d.sizes, st.d.off[0], st.units};
        return e;
    }
    st.up.done(stream);
    return e;
}

// ---- matrepair_ragged dispatch ----------------------------------------------------------
const KrNames g_ragged_repair_names("matrepair_ragged");

// The staged head of a ragged repair: the records, then the ids the call staged
// (host-side ones, or none given: every stripe pattern 0), each padded to 256 bytes.
size_t ragged_repair_tab_bytes(const RaggedRepairSpec& p) {
    return (size_t(p.npatterns) * repair_rec_dwords(p.k, p.t) * 4 + 255) / 256 * 256;
}

// Rows [g0, g0 + R) of every stripe.
struct RaggedRepairKr {
    template <int K, int R>
    static hipError_t launch(const RaggedRepairSpec& p, const RaggedDev& d, uint32_t g0, uint32_t grid,
                             hipStream_t stream) {
        RaggedRepairJob job;
        job.in_bstride = p.in_bstride;
        job.out_bstride = p.out_bstride;
        job.in_bytes = p.in_bytes;
        job.out_bytes = p.out_bytes;
        job.nstripes = static_cast<uint32_t>(p.nstripes);
        job.rows_all = p.t;
        job.row0 = g0;
        job.npatterns = p.npatterns;
        job.rec_dwords = repair_rec_dwords(K, p.t);
        job.tab_off = g0 * K * 5;
        job.mask_off = p.t * K * 5;
        job.pad_ = 0;
        job.ustart = d.ustart;
        job.sizes = d.sizes;
        job.in_off = d.off[0];
        job.out_off = d.off[1];
        job.records = reinterpret_cast<const uint32_t*>(d.head);
        job.ids = p.ids_dev ? p.ids_dev : reinterpret_cast<const uint32_t*>(d.head + ragged_repair_tab_bytes(p));
        job.in = p.in;
        job.out = p.out;
        const hipError_t e =
            launch_job(reinterpret_cast<const void*>(matrepair_ragged<K, R>), grid, kBlock, 0, stream, job);
        if (e == hipSuccess) t_last_kernel = g_ragged_repair_names.name[K][R];
        return e;
    }
};
constexpr KrTable<RaggedRepairKr> g_ragged_repair_launch;

// RaggedStage with a head of [records | ids (host-side or none given)].  The grid rule is
// matapply_ragged's, ceil(10 / (k + r)) units per wave, r the most live rows
// any pattern has within the launch's row group; a row group no pattern uses
// is skipped.
hipError_t launch_ragged_repair_all(const RaggedRepairSpec& p, hipStream_t stream) {
    const uint64_t ns = p.nstripes;
    const uint32_t k = p.k, t = p.t;
    const uint32_t any = repair_any(p.masks, p.npatterns, t);
    if (!any) return hipSuccess;  // nothing to store: no upload, no launch
    const size_t tab_bytes = ragged_repair_tab_bytes(p);
    const bool stage_ids = !p.ids_dev;  // host-side ids, or none: every stripe pattern 0
    const size_t ids_bytes = stage_ids ? (size_t(ns) * 4 + 255) / 256 * 256 : 0;
    const auto fill_head = [&](uint8_t* host) {
        repair_fill_records(reinterpret_cast<uint32_t*>(host), p.rows, p.masks, p.npatterns, k, t);
        if (!stage_ids) return;
        if (p.ids_host)
            std::memcpy(host + tab_bytes, p.ids_host, size_t(ns) * 4);
        else
            std::memset(host + tab_bytes, 0, size_t(ns) * 4);
    };
    RaggedStage st;
    hipError_t e = st.stage(p.sizes, {p.in_off, p.out_off}, ns, p.desc_host, std::min(p.in_bytes, p.out_bytes),
                            std::min(ragged_units_bound(p.in_bytes, p.in_bstride, k),
                                     ragged_units_bound(p.out_bytes, p.out_bstride, t)),
                            tab_bytes + ids_bytes, fill_head, stream);
    if (e != hipSuccess || !st.units) return e;
    for (uint32_t g0 = 0; g0 < t && e == hipSuccess; g0 += kRegR) {
        const uint32_t rg = std::min<uint32_t>(kRegR, t - g0);
        uint32_t rmax = 0;  // the most live rows any pattern has in this group
        for (size_t q = 0; q < p.npatterns; ++q)
            rmax = std::max<uint32_t>(rmax, __builtin_popcount((p.masks[q] >> g0) & ((1u << rg) - 1u)));
        if (!rmax) continue;  // rows no pattern stores
        e = g_ragged_repair_launch(k, rg)(p, st.d, g0, ragged_grid(st.units, ragged_units_per_wave(k, rmax)), stream);
    }
    st.up.done(stream);
    return e;
}

// ---- matupdate_ragged dispatch ----------------------------------------------------------
const KrNames g_ragged_update_names("matupdate_ragged");

// The staged head of a ragged update: matupdate_reg's k records, then the
// host-side numbers, each padded to 256 bytes.
size_t ragged_update_tab_bytes(const RaggedUpdateSpec& p) {
    return (size_t(p.k) * update_rec_dwords(p.nrows) * 4 + 255) / 256 * 256;
}

// Rows [g0, g0 + R) of every stripe; K is the number of input slots.
struct RaggedUpdateKr {
    template <int K, int R>
    static hipError_t launch(const RaggedUpdateSpec& p, const RaggedDev& d, uint32_t g0, uint32_t grid,
                             hipStream_t stream) {
        RaggedUpdateJob job;
        job.in_bstride = p.in_bstride;
        job.row_bstride = p.row_bstride;
        job.in_bytes = p.in_bytes;
        job.row_bytes = p.row_bytes;
        job.nstripes = static_cast<uint32_t>(p.nstripes);
        job.rows_all = p.nrows;
        job.row0 = g0;
        job.k = p.k;
        job.rec_dwords = update_rec_dwords(p.nrows);
        job.tab_off = g0 * 5;
        job.mask_off = p.nrows * 5 + g0 / 32;
        job.bit0 = g0 % 32;
        job.ustart = d.ustart;
        job.sizes = d.sizes;
        job.in_off = d.off[0];
        job.row_off = d.off[1];
        job.records = reinterpret_cast<const uint32_t*>(d.head);
        job.changed =
            p.changed_dev ? p.changed_dev : reinterpret_cast<const uint32_t*>(d.head + ragged_update_tab_bytes(p));
        job.nw = p.newb;
        job.od = p.oldb;
        job.rows = p.rows;
        const hipError_t e =
            launch_job(reinterpret_cast<const void*>(matupdate_ragged<K, R>), grid, kBlock, 0, stream, job);
        if (e == hipSuccess) t_last_kernel = g_ragged_update_names.name[K][R];
        return e;
    }
};
constexpr KrTable<RaggedUpdateKr> g_ragged_update_launch;

// RaggedStage with a head of [records | host-side numbers].  The grid rule is
// matapply_ragged's over the blocks a unit really moves: c inputs (2 c with old
// bytes) and the launch's rows twice, read and written.  No row group can be
// empty: a parity row's coefficients are never zero, and a primary row is live
// for the stripes that change it.
hipError_t launch_ragged_update_all(const RaggedUpdateSpec& p, hipStream_t stream) {
    const uint64_t ns = p.nstripes;
    const size_t tab_bytes = ragged_update_tab_bytes(p);
    const size_t ch_bytes = p.changed_host ? (size_t(ns) * p.c * 4 + 255) / 256 * 256 : 0;
    const auto fill_head = [&](uint8_t* host) {
        update_fill_records(reinterpret_cast<uint32_t*>(host), p.coefs, p.k, p.nrows);
        if (ch_bytes) std::memcpy(host + tab_bytes, p.changed_host, size_t(ns) * p.c * 4);
    };
    RaggedStage st;
    hipError_t e = st.stage(p.sizes, {p.in_off, p.row_off}, ns, p.desc_host, std::min(p.in_bytes, p.row_bytes),
                            std::min(ragged_units_bound(p.in_bytes, p.in_bstride, p.c),
                                     ragged_units_bound(p.row_bytes, p.row_bstride, p.nrows)),
                            tab_bytes + ch_bytes, fill_head, stream);
    if (e != hipSuccess || !st.units) return e;
    const uint32_t moved_in = p.c * (p.oldb ? 2u : 1u);
    for (uint32_t g0 = 0; g0 < p.nrows && e == hipSuccess; g0 += kRegR) {
        const uint32_t rg = std::min<uint32_t>(kRegR, p.nrows - g0);
        e = g_ragged_update_launch(p.c, rg)(p, st.d, g0, ragged_grid(st.units, ragged_units_per_wave(moved_in, 2 * rg)),
                                            stream);
    }
    st.up.done(stream);
    return e;
}

// ---- mix form of the run-time-data bit-sliced kernels (4 < k <= 32) ------------------
// Waves (row tiles) per unit from r alone -- not from the size of the call as
// bsr_tiles -- so that a record serves every call: one wave for r <= 10, 2 for
// r <= 20, 4 for r <= 32, tiles of rt = ceil(r / nw) rows.
void bsr_mix_tiles(uint32_t r, uint32_t* nw, uint32_t* rt) {
    *nw = r <= static_cast<uint32_t>(kBsrMaxRows) ? 1u : r <= 2u * kBsrMaxRows ? 2u : 4u;
    *rt = (r + *nw - 1) / *nw;
}

// uint64 words per record: the addresses, the mask dword, padded to 16 bytes.
uint32_t bsr_mix_stride(uint32_t k, uint32_t r) {
    uint32_t nw, rt;
    bsr_mix_tiles(r, &nw, &rt);
    return (nw * k * rt + 1 + 1) / 2 * 2;
}

struct BsrMixVariant {
    const void* fn_solo = nullptr;
    const void* fn = nullptr;  // LDS-phase form: RT 6-10 (r = 11..32 on 2 or 4 waves)
    KName name_solo = "";
    KName name = "";
};
BsrMixVariant g_bsr_mix[kBsrMaxRows + 1];
std::once_flag g_bsr_mix_once;

void fill_bsr_mix() {
    for_each_rt<kBsrMaxRows>([](auto rt) {
        constexpr int RT = decltype(rt)::value;
        BsrMixVariant& v = g_bsr_mix[RT];
        v.fn_solo = reinterpret_cast<const void*>(matapply_bsr_mix_solo<RT>);
        kname(v.name_solo, "matapply_bsr", RT, ",mix");
        if constexpr (RT >= 6) {
            v.fn = reinterpret_cast<const void*>(matapply_bsr<RT, true, false, BsrMixJob>);
            kname(v.name, "matapply_bsr", RT, ",lds,mix");
        }
    });
}

// launch_mixed / launch_repair for 4 < k <= 32: the records of every pattern
// and any host-side ids through one staging slot, then one launch.  Every way
// to decline comes before anything is enqueued.
hipError_t launch_repair_wide(const RepairSpec& p, hipStream_t stream) {
    if (!repair_any(p.masks, p.npatterns, p.t)) return hipSuccess;  // nothing to store: no upload, no launch
    const size_t rec = bsr_mix_record_bytes(p.k, p.t);
    if (!bsr_mix_ok(p.k, p.t, p.sz) || rec * p.npatterns > kBsrMixMaxBytes) return hipErrorNotSupported;
    const uint64_t cps = (p.sz + kBsrChunk - 1) / kBsrChunk;
    if (cps >= (1ull << 32) || p.nstripes >= (1ull << 32) || cps * p.nstripes >= (1ull << 32) - (1ull << 24))
        return hipErrorNotSupported;
    uint64_t base = 0;
    if (bsr_routine_base(&base, stream) != hipSuccess) return hipErrorNotSupported;
    const size_t tab_bytes = (rec * p.npatterns + 255) / 256 * 256;
    const size_t ids_bytes = p.ids_host ? size_t(p.nstripes) * 4 : 0;
    StagedUpload up;
    hipError_t e = up.acquire(tab_bytes + ids_bytes);
    if (e != hipSuccess) return e;
    if (!bsr_mix_fill_records(up.host(), p.rows, p.masks, p.npatterns, p.k, p.t, base)) return hipErrorInvalidValue;
    if (ids_bytes) std::memcpy(up.host() + tab_bytes, p.ids_host, ids_bytes);
    if ((e = up.copy(tab_bytes + ids_bytes, stream)) != hipSuccess) return e;
    BsrMixSpec m;
    m.k = p.k;
    m.r = p.t;
    m.npatterns = p.npatterns;
    m.records = up.dev();
    m.ids = p.ids_host ? reinterpret_cast<const uint32_t*>(up.dev() + tab_bytes) : p.ids_dev;
    m.in = p.in;
    m.out = p.out;
    m.sz = p.sz;
    m.nstripes = p.nstripes;
    m.in_sstride = p.in_sstride;
    m.out_sstride = p.out_sstride;
    e = launch_bsr_mixed(m, stream);
    up.done(stream);
    return e;
}

}  // namespace

bool bsr_mix_ok(uint32_t k, uint32_t r, uint64_t sz) {
    return generic_mode() == 2 && k > kMixedMaxK && k <= static_cast<uint32_t>(kMaxIn) && r >= 1 &&
           r <= kRepairMaxRows && sz >= kBsrChunk;
}

size_t bsr_mix_record_bytes(uint32_t k, uint32_t r) { return size_t(bsr_mix_stride(k, r)) * 8; }

bool bsr_mix_fill_records(void* dst, const uint8_t* rows, const uint32_t* masks, size_t npatterns, uint32_t k,
                          uint32_t r, uint64_t base) {
    uint32_t nw, rt;
    bsr_mix_tiles(r, &nw, &rt);
    const uint32_t stride = bsr_mix_stride(k, r), naddr = nw * k * rt;
    const uint32_t all = r < 32 ? (1u << r) - 1u : ~0u;
    ApplySpec a{};
    a.k = k;
    a.r = r;
    a.coef_stride = k;
    for (size_t q = 0; q < npatterns; ++q) {
        uint64_t* rec = static_cast<uint64_t*>(dst) + q * stride;
        a.coef = rows + q * r * k;
        if (!fill_bsr_addrs(rec, a, base, 1, nw, rt, 1)) return false;
        for (uint32_t i = naddr; i < stride; ++i) rec[i] = 0;
        rec[naddr] = (masks ? masks[q] : all) & all;  // the mask is the low dword
    }
    return true;
}

hipError_t launch_bsr_mixed(const BsrMixSpec& m, hipStream_t stream) {
    std::call_once(g_dispatch_once, init_dispatch);
    std::call_once(g_bsr_mix_once, fill_bsr_mix);
    if (!m.records || !m.ids || m.npatterns < 1 || m.nstripes == 0 || m.nstripes >= (1ull << 32))
        return hipErrorInvalidValue;
    if (!bsr_mix_ok(m.k, m.r, m.sz)) return hipErrorNotSupported;
    uint64_t base = 0;
    if (bsr_routine_base(&base, stream) != hipSuccess) return hipErrorNotSupported;
    const uint64_t cps = (m.sz + kBsrChunk - 1) / kBsrChunk;
    const uint64_t units = cps * m.nstripes;
    if (units >= (1ull << 32) - (1ull << 24)) return hipErrorNotSupported;
    uint32_t nw, rt;
    bsr_mix_tiles(m.r, &nw, &rt);
    const BsrMixVariant& v = g_bsr_mix[rt];
    if (nw > 1 && !v.fn) return hipErrorNotSupported;
    reset_signal();
    BsrMixJob job;
    job.sz = m.sz;
    job.in_sstride = m.in_sstride;
    job.out_sstride = m.out_sstride;
    job.nstripes = static_cast<uint32_t>(m.nstripes);
    job.k = m.k;
    job.r = m.r;
    const uint32_t grid = fill_stride(job, cps, units, bsr_grid_cap());
    job.npatterns = m.npatterns;
    job.stride = bsr_mix_stride(m.k, m.r);
    job.ids = m.ids;
    job.records = static_cast<const uint64_t*>(m.records);
    for (uint32_t j = 0; j < m.k; ++j) job.ptr[j] = m.in[j];
    for (uint32_t i = 0; i < m.r; ++i) job.ptr[m.k + i] = m.out[i];
    const hipError_t e = nw == 1 ? launch_job(v.fn_solo, grid, 64, 0, stream, job)
                                 : launch_job(v.fn, grid, 64 * nw, bsr_lds_bytes(m.k, nw, false), stream, job);
    if (e == hipSuccess) t_last_kernel = nw == 1 ? v.name_solo : v.name;
    return e;
}

size_t repair_records_bytes(uint32_t k, uint32_t t, size_t npatterns) {
    if (k < 1 || k > static_cast<uint32_t>(kMaxIn) || t < 1 || t > kRepairMaxRows) return 0;
    return npatterns * (k <= kMixedMaxK ? size_t(repair_rec_dwords(k, t)) * 4 : bsr_mix_record_bytes(k, t));
}

hipError_t repair_records_fill(void* dst, const uint8_t* rows, const uint32_t* masks, size_t npatterns, uint32_t k,
                               uint32_t t) {
    if (!repair_records_bytes(k, t, npatterns)) return hipErrorNotSupported;
    if (k <= kMixedMaxK) {
        repair_fill_records(static_cast<uint32_t*>(dst), rows, masks, npatterns, k, t);
        return hipSuccess;
    }
    uint64_t base = 0;
    if (bsr_routine_base(&base, nullptr) != hipSuccess) return hipErrorNotSupported;
    return bsr_mix_fill_records(dst, rows, masks, npatterns, k, t, base) ? hipSuccess : hipErrorInvalidValue;
}

hipError_t launch_repair_records(const RepairSpec& p, const void* records, hipStream_t stream) {
    std::call_once(g_dispatch_once, init_dispatch);
    if (p.k < 1 || p.k > static_cast<uint32_t>(kMaxIn) || p.t < 1 || p.t > kRepairMaxRows || p.npatterns < 1 ||
        !p.masks || !records || (!p.ids_host && !p.ids_dev) || p.sz == 0 || p.nstripes == 0 ||
        p.nstripes >= (1ull << 32))
        return hipErrorInvalidValue;
    const uint32_t any = repair_any(p.masks, p.npatterns, p.t);
    if (!any) return hipSuccess;  // nothing to store: no launch
    const bool wide = p.k > kMixedMaxK;
    if (wide) {  // every way to decline, before anything is enqueued
        const uint64_t cps = (p.sz + kBsrChunk - 1) / kBsrChunk;
        uint64_t base = 0;
        if (!bsr_mix_ok(p.k, p.t, p.sz) || cps >= (1ull << 32) ||
            cps * p.nstripes >= (1ull << 32) - (1ull << 24) || bsr_routine_base(&base, stream) != hipSuccess)
            return hipErrorNotSupported;
    }
    const uint32_t* ids = p.ids_dev;
    StagedUpload up;
    if (p.ids_host) {  // the ids alone through a staging slot
        if (stream_capturing(stream)) return hipErrorNotSupported;
        const size_t ids_bytes = size_t(p.nstripes) * 4;
        hipError_t e = up.acquire(ids_bytes);
        if (e != hipSuccess) return e;
        std::memcpy(up.host(), p.ids_host, ids_bytes);
        if ((e = up.copy(ids_bytes, stream)) != hipSuccess) return e;
        ids = reinterpret_cast<const uint32_t*>(up.dev());
    }
    reset_signal();
    hipError_t e;
    if (wide) {
        BsrMixSpec m;
        m.k = p.k;
        m.r = p.t;
        m.npatterns = p.npatterns;
        m.records = records;
        m.ids = ids;
        m.in = p.in;
        m.out = p.out;
        m.sz = p.sz;
        m.nstripes = p.nstripes;
        m.in_sstride = p.in_sstride;
        m.out_sstride = p.out_sstride;
        e = launch_bsr_mixed(m, stream);
    } else {
        e = launch_repair_groups(p, static_cast<const uint32_t*>(records), ids, any, stream);
    }
    if (p.ids_host) up.done(stream);
    return e;
}

hipError_t launch_repair(const RepairSpec& p, hipStream_t stream) {
    std::call_once(g_dispatch_once, init_dispatch);
    if (p.k < 1 || p.k > static_cast<uint32_t>(kMaxIn) || p.t < 1 || p.t > kRepairMaxRows || p.npatterns < 1 ||
        p.npatterns > kMixedMaxPatterns || !p.rows || !p.masks || (!p.ids_host && !p.ids_dev) || p.sz == 0 ||
        p.nstripes == 0 || p.nstripes >= (1ull << 32))
        return hipErrorInvalidValue;
    if (stream_capturing(stream)) return hipErrorNotSupported;
    reset_signal();
    if (p.k > kMixedMaxK) return launch_repair_wide(p, stream);
    return launch_repair_all(p, stream);
}

hipError_t launch_update(const UpdateSpec& p, hipStream_t stream) {
    static_assert(kUpdateMaxSlots == uint32_t(kRegK), "one matupdate_reg<C, R> per slot count");
    std::call_once(g_dispatch_once, init_dispatch);
    if (p.k < 1 || p.nrows < 1 || p.nrows > kUpdateMaxRows || p.c < 1 || p.c > kUpdateMaxSlots || !p.coefs ||
        (!p.changed_host && !p.changed_dev) || !p.newb || !p.rows || p.sz == 0 || p.nstripes == 0 ||
        p.nstripes >= (1ull << 32))
        return hipErrorInvalidValue;
    if (stream_capturing(stream)) return hipErrorNotSupported;
    reset_signal();
    return launch_update_all(p, stream);
}

hipError_t launch_verify(const VerifySpec& v, hipStream_t stream) {
    std::call_once(g_dispatch_once, init_dispatch);
    if (v.k < 1 || v.k > static_cast<uint32_t>(kRegK) || v.r < 1 || v.r > static_cast<uint32_t>(kRegR) ||
        v.coef_stride < v.k || !v.mismatch || v.sz == 0 || v.nstripes == 0 || v.nstripes >= (1ull << 32) ||
        uint64_t(v.bit0) + v.r > uint64_t(v.words) * 32)
        return hipErrorInvalidValue;
    reset_signal();
    return g_verify_launch(v.k, v.r)(v, stream);
}

bool verify_bsr_ok(uint32_t k, uint32_t r, uint64_t sz) {
    return k > 4 && r >= 1 && bsr_shape_ok(k, r < kVerifyBsrRows ? r : kVerifyBsrRows, sz);
}

hipError_t launch_verify_bsr(const VerifySpec& v, hipStream_t stream) {
    std::call_once(g_dispatch_once, init_dispatch);
    if (!v.mismatch || v.coef_stride < v.k || v.nstripes == 0 || v.nstripes >= (1ull << 32) ||
        uint64_t(v.bit0) + v.r > uint64_t(v.words) * 32)
        return hipErrorInvalidValue;
    if (v.r > kVerifyBsrRows || !verify_bsr_ok(v.k, v.r, v.sz)) return hipErrorNotSupported;
    reset_signal();
    return launch_verify_bsr_one(v, stream);
}

hipError_t launch_rows_differ(const DifferSpec& d, hipStream_t stream) {
    std::call_once(g_dispatch_once, init_dispatch);
    if (d.r < 1 || d.r > static_cast<uint32_t>(kMaxOut) || !d.mismatch || d.sz == 0 || d.nstripes == 0 ||
        d.nstripes >= (1ull << 32) || uint64_t(d.bit0) + d.r > uint64_t(d.words) * 32)
        return hipErrorInvalidValue;
    reset_signal();
    DifferJob job;
    job.a_sstride = d.a_sstride;
    job.b_sstride = d.b_sstride;
    job.words = d.words;
    job.bit0 = d.bit0;
    job.r = d.r;
    for (uint32_t i = d.r; i < static_cast<uint32_t>(kMaxOut); ++i) job.a[i] = job.b[i] = nullptr;
    const hipError_t e = launch_pieces(d.sz, d.nstripes, [&](uint64_t b0, uint64_t len, uint64_t s0, uint64_t ns) {
        const uint32_t grid = fill_walk(job.walk, len, ns);
        job.mismatch = d.mismatch + s0 * d.words;
        for (uint32_t i = 0; i < d.r; ++i) {
            job.a[i] = d.a[i] + b0 + s0 * d.a_sstride;
            job.b[i] = d.b[i] + b0 + s0 * d.b_sstride;
        }
        return launch_job(reinterpret_cast<const void*>(rows_differ), grid, kBlock, 0, stream, job);
    });
    if (e == hipSuccess) t_last_kernel = "rows_differ";
    return e;
}

hipError_t launch_locate(const VerifySpec& v, const uint8_t* q, uint32_t xbit, hipStream_t stream) {
    std::call_once(g_dispatch_once, init_dispatch);
    if (v.k < 1 || v.k > static_cast<uint32_t>(kRegK) || v.r < 2 || v.r > static_cast<uint32_t>(kRegR) ||
        v.coef_stride < v.k || !q || !v.mismatch || v.sz == 0 || v.nstripes == 0 || v.nstripes >= (1ull << 32) ||
        v.bit0 != 0 || v.r > xbit || uint64_t(xbit) + v.k > uint64_t(v.words) * 32)
        return hipErrorInvalidValue;
    reset_signal();
    return g_locate_launch(v.k, v.r)(v, LocateArgs{q, xbit}, stream);
}

// The n tables of `coefs` into device memory, by one staged upload.
static hipError_t upload_tabs(StagedUpload& up, const uint8_t* coefs, size_t n, hipStream_t stream) {
    const hipError_t e = up.acquire(n * 5 * sizeof(uint32_t));
    if (e != hipSuccess) return e;
    uint32_t* ht = reinterpret_cast<uint32_t*>(up.host());
    for (size_t i = 0; i < n; ++i) host_tab(ht + i * 5, coefs[i]);
    return up.copy(n * 5 * sizeof(uint32_t), stream);
}

hipError_t locate_tables_upload(const uint8_t* q, uint32_t k, uint32_t c, hipStream_t stream, LocateTables* out) {
    if (!q || !out || k < 1 || c < 2) return hipErrorInvalidValue;
    if (stream_capturing(stream)) return hipErrorNotSupported;
    StagedUpload up;
    const hipError_t e = upload_tabs(up, q, size_t(k) * (c - 1), stream);
    if (e != hipSuccess) return e;
    out->dev = reinterpret_cast<const uint32_t*>(up.dev());
    out->slot = up.slot;
    return hipSuccess;
}

void locate_tables_release(const LocateTables& t, hipStream_t stream) {
    if (t.slot) StagedUpload{static_cast<Slot*>(t.slot)}.done(stream);
}

hipError_t launch_rows_locate(const DifferSpec& d, const uint8_t* a0, const uint8_t* b0, uint32_t k, uint32_t xbit,
                              const uint32_t* qtab_dev, hipStream_t stream) {
    std::call_once(g_dispatch_once, init_dispatch);
    if (d.r < 1 || d.r > static_cast<uint32_t>(kMaxOut) || !d.mismatch || !a0 || !b0 || !qtab_dev || k < 1 ||
        d.sz == 0 || d.nstripes == 0 || d.nstripes >= (1ull << 32) || uint64_t(d.bit0) + d.r > xbit ||
        uint64_t(xbit) + k > uint64_t(d.words) * 32)
        return hipErrorInvalidValue;
    reset_signal();
    LocateRowsJob job;
    job.a_sstride = d.a_sstride;
    job.b_sstride = d.b_sstride;
    job.words = d.words;
    job.bit0 = d.bit0;
    job.r = d.r;
    job.k = k;
    job.xbit = xbit;
    job.pad_ = 0;
    job.qtab = qtab_dev;
    for (uint32_t i = d.r; i < static_cast<uint32_t>(kMaxOut); ++i) job.a[i] = job.b[i] = nullptr;
    const hipError_t e = launch_pieces(d.sz, d.nstripes, [&](uint64_t b0off, uint64_t len, uint64_t s0, uint64_t ns) {
        const uint32_t grid = fill_walk(job.walk, len, ns);
        job.bits = d.mismatch + s0 * d.words;
        job.a0 = a0 + b0off + s0 * d.a_sstride;
        job.b0 = b0 + b0off + s0 * d.b_sstride;
        for (uint32_t i = 0; i < d.r; ++i) {
            job.a[i] = d.a[i] + b0off + s0 * d.a_sstride;
            job.b[i] = d.b[i] + b0off + s0 * d.b_sstride;
        }
        return launch_job(reinterpret_cast<const void*>(rows_locate), grid, kBlock, 0, stream, job);
    });
    if (e == hipSuccess) t_last_kernel = "rows_locate";
    return e;
}

hipError_t launch_locate_finish(const uint32_t* bits, uint32_t words, uint32_t k, uint32_t c, uint64_t nstripes,
                                uint32_t* culprit, hipStream_t stream) {
    std::call_once(g_dispatch_once, init_dispatch);
    if (!bits || !culprit || k < 1 || c < 1 || nstripes == 0 || nstripes >= (1ull << 32) ||
        words != (c + 31) / 32 + (k + 31) / 32)
        return hipErrorInvalidValue;
    FinishJob job;
    job.bits = bits;
    job.culprit = culprit;
    job.nstripes = static_cast<uint32_t>(nstripes);
    job.k = k;
    job.c = c;
    job.words = words;
    const uint32_t grid = static_cast<uint32_t>((nstripes + kBlock - 1) / kBlock);
    return launch_job(reinterpret_cast<const void*>(locate_finish), grid, kBlock, 0, stream, job);
}

hipError_t launch_correct(const CorrectSpec& p, hipStream_t stream) {
    static const char* const kNames[kRegK + 1] = {"", "matcorrect_reg<1>", "matcorrect_reg<2>", "matcorrect_reg<3>",
                                                  "matcorrect_reg<4>"};
    static const void* const kFns[kRegK + 1] = {
        nullptr, reinterpret_cast<const void*>(matcorrect_reg<1>), reinterpret_cast<const void*>(matcorrect_reg<2>),
        reinterpret_cast<const void*>(matcorrect_reg<3>), reinterpret_cast<const void*>(matcorrect_reg<4>)};
    std::call_once(g_dispatch_once, init_dispatch);
    if (p.k < 1 || p.nb <= p.k || p.nb > 256 || !p.rows || !p.verdict || !p.blocks || p.sz == 0 || p.nstripes == 0 ||
        p.nstripes >= (1ull << 32))
        return hipErrorInvalidValue;
    if (stream_capturing(stream)) return hipErrorNotSupported;
    reset_signal();
    const bool reg = p.k <= static_cast<uint32_t>(kRegK);
    StagedUpload up;
    hipError_t e = upload_tabs(up, p.rows, size_t(p.nb) * p.k, stream);
    if (e != hipSuccess) return e;
    CorrectJob job;
    job.bstride = p.bstride;
    job.sstride = p.sstride;
    job.k = p.k;
    job.nb = p.nb;
    job.tabs = reinterpret_cast<const uint32_t*>(up.dev());
    const void* const fn = reg ? kFns[p.k] : reinterpret_cast<const void*>(rows_correct);
    e = launch_pieces(p.sz, p.nstripes, [&](uint64_t b0, uint64_t len, uint64_t s0, uint64_t ns) {
        const uint32_t grid = fill_walk(job.walk, len, ns);
        job.verdict = p.verdict + s0;
        job.blocks = p.blocks + b0 + s0 * p.sstride;
        return launch_job(fn, grid, kBlock, 0, stream, job);
    });
    up.done(stream);
    if (e == hipSuccess) t_last_kernel = reg ? kNames[p.k] : "rows_correct";
    return e;
}

hipError_t launch_locate2_finish(const uint32_t* bits, uint32_t words, uint32_t k, uint32_t c, uint64_t nstripes,
                                 uint32_t* culprit, uint32_t* list, uint32_t* pairbits, hipStream_t stream,
                                 uint64_t plane) {
    std::call_once(g_dispatch_once, init_dispatch);
    if (!bits || !culprit || k < 1 || c < 1 || nstripes == 0 || nstripes >= (1ull << 32) ||
        words != (c + 31) / 32 + (k + 31) / 32 || (list != nullptr) != (pairbits != nullptr) ||
        (list && !pairs_shape_ok(k, c)) || (plane && plane < nstripes) || plane >= (1ull << 32))
        return hipErrorInvalidValue;
    Finish2Job job;
    job.bits = bits;
    job.culprit = culprit;
    job.list = list;
    job.pairbits = pairbits;
    job.nstripes = static_cast<uint32_t>(nstripes);
    job.k = k;
    job.c = c;
    job.words = words;
    job.pw = list ? pairs_words(k + c) : 0u;
    job.plane = static_cast<uint32_t>(plane ? plane : nstripes);
    job.pad_[0] = job.pad_[1] = 0;
    const uint32_t grid = static_cast<uint32_t>((nstripes + kBlock - 1) / kBlock);
    return launch_job(reinterpret_cast<const void*>(locate2_finish), grid, kBlock, 0, stream, job);
}

namespace {
// The one upload of a pair pass: P's tables, the pairs' location records, then
// (sources and crows given) their correction records, the latter two at dword
// offsets *off_loc and *off_cor.
hipError_t pairs_upload(StagedUpload& up, uint32_t k, uint32_t c, const uint8_t* P, const uint8_t* pivots,
                        const uint32_t* sources, const uint8_t* crows, hipStream_t stream, size_t* off_loc,
                        size_t* off_cor) {
    const uint32_t nb = k + c, npairs = nb * (nb - 1) / 2;
    const bool heal = sources != nullptr;
    const size_t prec = 2 + 11 * size_t(c - 2), crec = 11 * size_t(k);
    *off_loc = size_t(c) * k * 5;
    *off_cor = *off_loc + npairs * prec;
    const size_t dwords = *off_cor + (heal ? npairs * crec : 0);
    hipError_t e = up.acquire(dwords * sizeof(uint32_t));
    if (e != hipSuccess) return e;
    uint32_t* const ht = reinterpret_cast<uint32_t*>(up.host());
    for (size_t i = 0; i < size_t(c) * k; ++i) host_tab(ht + i * 5, P[i]);
    const size_t pbytes = 2 + 3 * size_t(c - 2);
    for (uint32_t q = 0; q < npairs; ++q) {
        const uint8_t* src = pivots + q * pbytes;
        uint32_t* dst = ht + *off_loc + q * prec;
        dst[0] = src[0];
        dst[1] = src[1];
        for (uint32_t m = 0; m + 2 < c; ++m) {
            dst[2 + 11 * m] = src[2 + 3 * m];
            host_tab(dst + 2 + 11 * m + 1, src[2 + 3 * m + 1]);
            host_tab(dst + 2 + 11 * m + 6, src[2 + 3 * m + 2]);
        }
        if (!heal) continue;
        dst = ht + *off_cor + q * crec;
        for (uint32_t l = 0; l < k; ++l) dst[l] = sources[size_t(q) * k + l];
        for (uint32_t l = 0; l < 2 * k; ++l) host_tab(dst + k + 5 * l, crows[size_t(q) * 2 * k + l]);
    }
    return up.copy(dwords * sizeof(uint32_t), stream);
}
}  // namespace

hipError_t launch_pairs(const PairsSpec& p, hipStream_t stream) {
    std::call_once(g_dispatch_once, init_dispatch);
    if (!pairs_shape_ok(p.k, p.c) || !p.P || !p.pivots || (p.sources != nullptr) != (p.crows != nullptr) ||
        !p.blocks || !p.list || !p.pairbits || !p.culprit || p.sz == 0 || p.nstripes == 0 ||
        p.nstripes >= (1ull << 32) || (p.plane && p.plane < p.nstripes) || p.plane >= (1ull << 32))
        return hipErrorInvalidValue;
    if (stream_capturing(stream)) return hipErrorNotSupported;
    reset_signal();
    const uint32_t k = p.k, c = p.c, nb = k + c, npairs = nb * (nb - 1) / 2;
    const bool heal = p.sources != nullptr;
    size_t off_loc, off_cor;
    StagedUpload up;
    hipError_t e = pairs_upload(up, k, c, p.P, p.pivots, p.sources, p.crows, stream, &off_loc, &off_cor);
    if (e != hipSuccess) return e;
    const uint32_t* const dev = reinterpret_cast<const uint32_t*>(up.dev());
    PairsJob job;
    job.bstride = p.bstride;
    job.sstride = p.sstride;
    job.k = k;
    job.c = c;
    job.nb = nb;
    job.npairs = npairs;
    job.pw = pairs_words(nb);
    job.plane = static_cast<uint32_t>(p.plane ? p.plane : p.nstripes);
    job.list = p.list;
    job.pairbits = p.pairbits;
    job.culprit = p.culprit;
    job.ptabs = dev;
    job.recs = dev + off_loc;
    job.blocks = p.blocks;
    // The host does not know the list's length: fixed grids, sized to fill the
    // device for a fully dirty batch, that walk grid-stride.  An empty list
    // costs every wave one scalar load.
    // one wave per workgroup, c KiB of LDS each
    uint32_t grid = fill_walk(job.walk, p.sz, p.nstripes, 1, hooked_grid_cap(uint64_t(g_num_cu) * 32));
    e = launch_job(reinterpret_cast<const void*>(pairs_locate), grid, 64, size_t(c) * 64 * sizeof(u32x4), stream, job);
    if (e == hipSuccess) {
        const uint64_t need = (p.nstripes + kBlock - 1) / kBlock, cap = hooked_grid_cap(uint64_t(g_num_cu) * 8);
        e = launch_job(reinterpret_cast<const void*>(pairs_finish), static_cast<uint32_t>(need < cap ? need : cap),
                       kBlock, 0, stream, job);
    }
    if (e == hipSuccess && heal) {
        job.recs = dev + off_cor;
        grid = fill_walk(job.walk, p.sz, p.nstripes, kBlock / 64, hooked_grid_cap(uint64_t(g_num_cu) * 8));
        e = launch_job(reinterpret_cast<const void*>(pairs_correct), grid, kBlock, 0, stream, job);
    }
    up.done(stream);
    if (e == hipSuccess) t_last_kernel = heal ? "pairs_correct" : "pairs_locate";
    return e;
}

hipError_t launch_pairs_ragged(const PairsRaggedSpec& p, hipStream_t stream) {
    std::call_once(g_dispatch_once, init_dispatch);
    if (!pairs_shape_ok(p.k, p.c) || !p.P || !p.pivots || (p.sources != nullptr) != (p.crows != nullptr) ||
        !p.blocks || !p.sizes || !p.off || !p.list || !p.pairbits || !p.culprit || p.nstripes == 0 ||
        p.nstripes >= (1ull << 32))
        return hipErrorInvalidValue;
    if (stream_capturing(stream)) return hipErrorNotSupported;
    reset_signal();
    const uint32_t k = p.k, c = p.c, nb = k + c, npairs = nb * (nb - 1) / 2;
    const bool heal = p.sources != nullptr;
    size_t off_loc, off_cor;
    StagedUpload up;
    hipError_t e = pairs_upload(up, k, c, p.P, p.pivots, p.sources, p.crows, stream, &off_loc, &off_cor);
    if (e != hipSuccess) return e;
    const uint32_t* const dev = reinterpret_cast<const uint32_t*>(up.dev());
    PairsRaggedJob rj;
    rj.bstride = p.bstride;
    rj.bytes = p.bytes;
    rj.nstripes = static_cast<uint32_t>(p.nstripes);
    rj.k = k;
    rj.c = c;
    rj.nb = nb;
    rj.npairs = npairs;
    rj.pw = pairs_words(nb);
    rj.sizes = p.sizes;
    rj.off = p.off;
    rj.list = p.list;
    rj.pairbits = p.pairbits;
    rj.culprit = p.culprit;
    rj.ptabs = dev;
    rj.recs = dev + off_loc;
    rj.blocks = p.blocks;
    // pairs_finish as it is: of its job it reads the list, the pair words, the planes and their stride
    PairsJob fj{};
    fj.k = k;
    fj.c = c;
    fj.nb = nb;
    fj.npairs = npairs;
    fj.pw = rj.pw;
    fj.plane = rj.nstripes;
    fj.list = p.list;
    fj.pairbits = p.pairbits;
    fj.culprit = p.culprit;
    // The host knows neither the list's length nor (device-side descriptors) a
    // listed stripe's size: the grids are the uniform pair pass's caps, or a wave
    // per work item where the whole batch has fewer, and the waves walk
    // grid-stride.  An empty list costs every wave one scalar load.
    const uint64_t items = p.nstripes * kPairSplit;
    uint64_t cap = hooked_grid_cap(uint64_t(g_num_cu) * 32);
    // one wave per workgroup, c KiB of LDS each
    e = launch_job(reinterpret_cast<const void*>(pairs_locate_ragged), static_cast<uint32_t>(std::min(items, cap)), 64,
                   size_t(c) * 64 * sizeof(u32x4), stream, rj);
    if (e == hipSuccess) {
        const uint64_t need = (p.nstripes + kBlock - 1) / kBlock;
        cap = hooked_grid_cap(uint64_t(g_num_cu) * 8);
        e = launch_job(reinterpret_cast<const void*>(pairs_finish), static_cast<uint32_t>(std::min(need, cap)), kBlock,
                       0, stream, fj);
    }
    if (e == hipSuccess && heal) {
        rj.recs = dev + off_cor;
        const uint64_t need = (items + kBlock / 64 - 1) / (kBlock / 64);
        e = launch_job(reinterpret_cast<const void*>(pairs_correct_ragged), static_cast<uint32_t>(std::min(need, cap)),
                       kBlock, 0, stream, rj);
    }
    up.done(stream);
    if (e == hipSuccess) t_last_kernel = heal ? "pairs_correct_ragged" : "pairs_locate_ragged";
    return e;
}

hipError_t launch_mixed(const MixedSpec& m, hipStream_t stream) {
    std::call_once(g_dispatch_once, init_dispatch);
    if (m.k < 1 || m.k > static_cast<uint32_t>(kMaxIn) || m.npatterns < 1 || m.npatterns > kMixedMaxPatterns ||
        !m.rows || (!m.ids_host && !m.ids_dev) || m.sz == 0 || m.nstripes == 0)
        return hipErrorInvalidValue;
    if (stream_capturing(stream)) return hipErrorNotSupported;
    reset_signal();
    if (m.k > kMixedMaxK) {  // a decode is a repair of the k primaries, every row live
        const std::vector<uint32_t> masks(m.npatterns, ~0u);
        RepairSpec p;
        p.k = p.t = m.k;
        p.rows = m.rows;
        p.masks = masks.data();
        p.npatterns = m.npatterns;
        p.ids_host = m.ids_host;
        p.ids_dev = m.ids_dev;
        p.in = m.in;
        p.out = m.out;
        p.sz = m.sz;
        p.nstripes = m.nstripes;
        p.in_sstride = m.in_sstride;
        p.out_sstride = m.out_sstride;
        return launch_repair_wide(p, stream);
    }
    switch (m.k) {
    case 1: return launch_mixed_k<1>(m, stream);
    case 2: return launch_mixed_k<2>(m, stream);
    case 3: return launch_mixed_k<3>(m, stream);
    default: return launch_mixed_k<4>(m, stream);
    }
}

hipError_t launch_ragged(const RaggedSpec& g, hipStream_t stream) {
    std::call_once(g_dispatch_once, init_dispatch);
    if (g.k < 1 || g.k > static_cast<uint32_t>(kRegK) || g.r < 1 || g.r > 256 || !g.coef || !g.in || !g.out ||
        !g.sizes || !g.in_off || !g.out_off || g.nstripes == 0 || g.nstripes >= (1ull << 32))
        return hipErrorInvalidValue;
    if (stream_capturing(stream)) return hipErrorNotSupported;
    reset_signal();
    return launch_ragged_all(g, stream);
}

hipError_t launch_ragged_scrub(const RaggedScrubSpec& p, hipStream_t stream) {
    std::call_once(g_dispatch_once, init_dispatch);
    const uint32_t cw = (p.c + 31) / 32;
    if (p.k < 1 || p.k > static_cast<uint32_t>(kRegK) || p.c < 1 || p.k + p.c > 256 || !p.P || !p.src || !p.sizes ||
        !p.off || !p.bits || p.nstripes == 0 || p.nstripes >= (1ull << 32) || p.words < cw ||
        (p.Q && (p.c < 2 || p.c > static_cast<uint32_t>(kRegR) || p.xbit < p.c ||
                 uint64_t(p.xbit) + p.k > uint64_t(p.words) * 32)))
        return hipErrorInvalidValue;
    if (stream_capturing(stream)) return hipErrorNotSupported;
    reset_signal();
    return launch_ragged_scrub_all(p, stream);
}

hipError_t launch_ragged_unfit(const uint64_t* sizes, const uint64_t* off, uint64_t nstripes, uint32_t slots,
                               uint64_t bstride, uint64_t bytes, uint32_t c, uint32_t* out, hipStream_t stream) {
    std::call_once(g_dispatch_once, init_dispatch);
    if (!sizes || !off || !out || slots < 1 || nstripes == 0 || nstripes >= (1ull << 32)) return hipErrorInvalidValue;
    UnfitJob job;
    job.sizes = sizes;
    job.off = off;
    job.bstride = bstride;
    job.bytes = bytes;
    job.out = out;
    job.nstripes = static_cast<uint32_t>(nstripes);
    job.slots = slots;
    job.words = (c + 31) / 32;
    job.c = c;
    const uint32_t grid = static_cast<uint32_t>((nstripes + kBlock - 1) / kBlock);
    return launch_job(reinterpret_cast<const void*>(ragged_unfit), grid, kBlock, 0, stream, job);
}

hipError_t launch_ragged_repair(const RaggedRepairSpec& p, hipStream_t stream) {
    std::call_once(g_dispatch_once, init_dispatch);
    if (p.k < 1 || p.k > static_cast<uint32_t>(kRegK) || p.t < 1 || p.t > kRepairMaxRows || p.npatterns < 1 ||
        p.npatterns > kMixedMaxPatterns || !p.rows || !p.masks || (p.ids_host && p.ids_dev) ||
        (!p.ids_host && !p.ids_dev && p.npatterns != 1) || !p.in || !p.out || !p.sizes || !p.in_off || !p.out_off ||
        p.nstripes == 0 || p.nstripes >= (1ull << 32))
        return hipErrorInvalidValue;
    if (stream_capturing(stream)) return hipErrorNotSupported;
    reset_signal();
    return launch_ragged_repair_all(p, stream);
}

hipError_t launch_ragged_update(const RaggedUpdateSpec& p, hipStream_t stream) {
    std::call_once(g_dispatch_once, init_dispatch);
    if (p.k < 1 || p.nrows < 1 || p.nrows > kUpdateMaxRows || p.c < 1 || p.c > kUpdateMaxSlots || !p.coefs ||
        (!p.changed_host == !p.changed_dev) || !p.newb || !p.rows || !p.sizes || !p.in_off || !p.row_off ||
        p.nstripes == 0 || p.nstripes >= (1ull << 32))
        return hipErrorInvalidValue;
    if (stream_capturing(stream)) return hipErrorNotSupported;
    reset_signal();
    return launch_ragged_update_all(p, stream);
}

void ragged_scrub_release(const RaggedScrubStaged& t, hipStream_t stream) {
    if (t.slot) StagedUpload{static_cast<Slot*>(t.slot)}.done(stream);
}

// ---- matcorrect_ragged dispatch ---------------------------------------------------------
hipError_t launch_ragged_correct(const RaggedCorrectSpec& p, hipStream_t stream) {
    std::call_once(g_dispatch_once, init_dispatch);
    if (p.k < 1 || p.k > static_cast<uint32_t>(kRegK) || p.nb <= p.k || p.nb > 256 || !p.rows || !p.verdict ||
        !p.blocks || !p.staged.ustart || !p.staged.sizes || !p.staged.off || p.nstripes == 0 ||
        p.nstripes >= (1ull << 32))
        return hipErrorInvalidValue;
    if (stream_capturing(stream)) return hipErrorNotSupported;
    reset_signal();
    static const char* const kNames[kRegK + 1] = {"", "matcorrect_ragged<1>", "matcorrect_ragged<2>",
                                                  "matcorrect_ragged<3>", "matcorrect_ragged<4>"};
    static const void* const kFns[kRegK + 1] = {nullptr, reinterpret_cast<const void*>(matcorrect_ragged<1>),
                                                reinterpret_cast<const void*>(matcorrect_ragged<2>),
                                                reinterpret_cast<const void*>(matcorrect_ragged<3>),
                                                reinterpret_cast<const void*>(matcorrect_ragged<4>)};
    StagedUpload up;
    hipError_t e = upload_tabs(up, p.rows, size_t(p.nb) * p.k, stream);
    if (e != hipSuccess) return e;
    RaggedCorrectJob job;
    job.bstride = p.bstride;
    job.bytes = p.bytes;
    job.nstripes = static_cast<uint32_t>(p.nstripes);
    job.nb = p.nb;
    job.ustart = p.staged.ustart;
    job.sizes = p.staged.sizes;
    job.off = p.staged.off;
    job.tabs = reinterpret_cast<const uint32_t*>(up.dev());
    job.verdict = p.verdict;
    job.blocks = p.blocks;
    // Not matapply_ragged's rule: a unit of a clean stripe moves no bytes, so a wave that owns few
    // units only pays for its search over ustart.  On 10^6 clean stripes of 4 KiB the call took 1.12 x
    // fec_correct_batch with 3 units per wave and 1.01 x with 48 (a ZFEC_HIP_GRID_CAP sweep that
    // slowed the location too), with every stripe corrupt 1.09 x and 1.05 x.
    constexpr uint64_t kCorrectUnitsPerWave = 48;
    e = launch_job(kFns[p.k], ragged_grid(std::max<uint64_t>(1, p.staged.units), kCorrectUnitsPerWave), kBlock, 0,
                   stream, job);
    up.done(stream);
    if (e == hipSuccess) t_last_kernel = kNames[p.k];
    return e;
}

int generic_mode() {
    int g = g_generic.load();
    if (g < 0) {
        const char* e = getenv("ZFEC_HIP_GENERIC");
        g = (e && e[0] >= '0' && e[0] <= '2') ? e[0] - '0' : 2;
        int expect = -1;
        if (!g_generic.compare_exchange_strong(expect, g)) g = expect;  // set_generic_mode won the race
    }
    return g;
}

void set_generic_mode(int mode) { g_generic.store(mode < 0 ? 0 : mode > 2 ? 2 : mode); }

const char* matapply_variant_name(uint32_t k, uint32_t r, bool accumulate) {
    if (!accumulate && k >= 1 && k <= static_cast<uint32_t>(kRegK) && r >= 1 && r <= static_cast<uint32_t>(kRegR))
        return kRegNames[k][r];
    return pick_lds(k, r, accumulate).name;
}

const char* matapply_last_kernel() { return t_last_kernel; }

void matapply_request_signal(uint32_t* flag_dev, uint32_t seq) {
    t_signal_flag = flag_dev;
    t_signal_seq = seq;
}

bool matapply_signal_used() { return t_signal_used; }

// Whether `stream` is being captured into a HIP graph.  The table forms read a
// device-side table the host fills (and reuses) at enqueue time: a captured
// graph would replay its copy from a host slot rewritten since, and the bsr
// address cache would hold a slot whose upload never ran (the copy is only
// recorded).  Under capture those forms decline (hipErrorNotSupported) and a
// kernel whose whole description travels in its arguments takes the launch.
bool stream_capturing(hipStream_t stream) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(stream, &st) == hipSuccess && st != hipStreamCaptureStatusNone;
}

bool wide_launch_ok(uint32_t k, uint32_t r, uint64_t sz, uint64_t nstripes) {
    // (forced) a specialised kernel of the whole matrix
    if (jit_mode() == kJitForce && sz >= static_cast<uint64_t>(kBsChunk) && k * r <= kJitMaxCoef) return true;
    // launches too small to fill the chip: matapply_small's passes of 32 inputs
    // (a wave per output row, every input load in flight at once) beat one
    // matapply_bsg launch walking all inputs in phases of 2
    if ((sz + 7) / 8 * nstripes < config().small_lanes) return false;
    return bsg_shape_ok(k, r, sz);  // matapply_bsg's table form
}

hipError_t launch_apply(const ApplySpec& a, hipStream_t stream) {
    uint32_t* const sig = t_signal_flag;  // a request covers this launch only
    reset_signal();
    std::call_once(g_dispatch_once, init_dispatch);
    const uint32_t k = a.k, r = a.r;
    const bool wide = k > static_cast<uint32_t>(kMaxIn);
    if (k == 0 || r == 0 || a.nstripes == 0 || a.sz == 0 || a.nstripes >= (1ull << 32) || a.coef_stride < k ||
        k > static_cast<uint32_t>(kMaxWideIn) || r > (wide ? 256u : static_cast<uint32_t>(kMaxOut)))
        return hipErrorInvalidValue;
    if (!wide && k * r > static_cast<uint32_t>(kMaxCoef)) return hipErrorInvalidValue;
    if (!a.accumulate) {  // a run-time specialised bit-sliced kernel, where one applies and is compiled
        const char* jit_name = nullptr;
        const hipError_t je = launch_matapply_jit(a, stream, &jit_name);
        if (je == hipSuccess) {
            t_last_kernel = jit_name;
            return hipSuccess;
        }
        if (je != hipErrorNotSupported && je != hipErrorNotReady) return je;
    }
    const bool reg = k <= static_cast<uint32_t>(kRegK) && r <= static_cast<uint32_t>(kRegR);
    if (wide) {
        if (a.accumulate || !bsg_shape_ok(k, r, a.sz)) return hipErrorNotSupported;
        // matapply_bsr, or matapply_bsg where it declines (hipErrorNotSupported:
        // a table past its ring slot, or no routine table on this device)
        hipError_t e = hipErrorNotSupported;
        if (bsr_wide_ok(k, r, a.sz, a.nstripes))
            e = launch_bsr_wide(a, stream);
        else if (bsr_tbl_ok(k, r, a.sz))
            e = launch_bsr_tbl(a, stream);
        if (e != hipErrorNotSupported) return e;
        return launch_bsg(a, stream);
    }
    const Config& cfg = config();
    if (!reg && (a.sz + 7) / 8 * a.nstripes < cfg.small_lanes) {
        MatJob job;
        fill_matjob(a, job);
        fill_coef(a, job);
        const hipError_t se = launch_small(job, stream);
        if (se != hipErrorNotSupported) {
            t_last_kernel = "matapply_small";
            return se;
        }
    }
    if (!a.accumulate) {
        hipError_t e = hipErrorNotSupported;
        if (bsr_shape_ok(k, r, a.sz))
            e = launch_bsr(a, stream);
        else if (bsr_tbl_ok(k, r, a.sz))
            e = launch_bsr_tbl(a, stream);
        if (e != hipErrorNotSupported) return e;
    }
    if (!a.accumulate && bsg_shape_ok(k, r, a.sz)) {
        const hipError_t e = launch_bsg(a, stream);
        if (e != hipErrorNotSupported) return e;  // (its table form declines under graph capture)
    }
    if (reg && !a.accumulate) return g_reg_launch[k][r](a, stream, sig);
    return launch_lds(a, stream);
}

hipError_t launch_one(const ApplySpec& a, hipStream_t stream, uint32_t* flag_dev, uint32_t seq,
                      const uint8_t* const* host_in, uint64_t host_sz) {
    static const char* const kOneNames[2][5] = {
        {"", "matapply_one<1>", "matapply_one<2>", "matapply_one<3>", "matapply_one<4>"},
        {"", "matapply_one<1,inline>", "matapply_one<2,inline>", "matapply_one<3,inline>", "matapply_one<4,inline>"}};
    if (a.k < 1 || a.k > 4 || a.r < 1 || a.r > 8 || a.nstripes != 1 || a.sz == 0 || a.sz % 16 || a.sz > 4096 ||
        a.accumulate || a.coef_stride < a.k)
        return hipErrorInvalidValue;
    reset_signal();
    const uint32_t units = static_cast<uint32_t>(a.sz / 16);
    // host_in: the caller has NOT copied the inputs anywhere the kernel can
    // read; they must fit the argument block, or the launch is refused (no
    // fallback to the bounce-buffer form, which would read stale memory)
    const bool inl = host_in != nullptr;
    if (inl && !one_inline_fits(a.k, a.sz, host_sz)) return hipErrorInvalidValue;
    thread_local OneJobInline big;  // ~5 KiB: not on the stack of every call
    OneJob& job = big.job;
    std::memset(&job, 0, sizeof job);
    for (uint32_t j = 0; j < a.k; ++j) job.in[j] = a.in[j];
    for (uint32_t i = 0; i < a.r; ++i) job.out[i] = a.out[i];
    job.done_flag = flag_dev;
    job.done_seq = seq;
    job.units = units;
    job.r = a.r;
    for (uint32_t i = 0; i < a.r; ++i)
        for (uint32_t j = 0; j < a.k; ++j) host_tab(&job.tab[(i * a.k + j) * 5], a.coef[size_t(i) * a.coef_stride + j]);
    typedef void (*OneFn)(const OneJob);
    typedef void (*OneInlFn)(const OneJobInline);
    static const OneFn kOne[5] = {nullptr, matapply_one<1, false, OneJob>, matapply_one<2, false, OneJob>,
                                  matapply_one<3, false, OneJob>, matapply_one<4, false, OneJob>};
    static const OneInlFn kOneInl[5] = {nullptr, matapply_one<1, true, OneJobInline>,
                                        matapply_one<2, true, OneJobInline>, matapply_one<3, true, OneJobInline>,
                                        matapply_one<4, true, OneJobInline>};
    t_last_kernel = kOneNames[inl ? 1 : 0][a.k];
    if (!inl) return launch_job(reinterpret_cast<const void*>(kOne[a.k]), 1, kBlock, 0, stream, job);
    // the caller's host blocks, each padded with zeros to its whole units
    uint8_t* d = reinterpret_cast<uint8_t*>(big.data);
    for (uint32_t j = 0; j < a.k; ++j) {
        std::memcpy(d + size_t(j) * units * 16, host_in[j], host_sz);
        std::memset(d + size_t(j) * units * 16 + host_sz, 0, size_t(units) * 16 - host_sz);
    }
    return launch_job(reinterpret_cast<const void*>(kOneInl[a.k]), 1, kBlock, 0, stream, big);
}

hipError_t launch_apply_pair(const ApplySpec& x, const ApplySpec& y, hipStream_t stream) {
    std::call_once(g_dispatch_once, init_dispatch);
    static std::once_flag names_once;
    std::call_once(names_once, [] {
        for (int k = 1; k <= kRegK; ++k)
            for (int ra = 1; ra <= kRegR; ++ra)
                for (int rb = 1; rb <= kRegR; ++rb)
                    snprintf(g_pair_names[k][ra][rb], sizeof g_pair_names[k][ra][rb], "matapply_pair<%d,%d,%d>", k,
                             ra, rb);
    });
    // the shapes launch_apply runs on matapply_reg (not matapply_rows, not a
    // forced JIT kernel), each within one launch
    auto reg_shape = [](const ApplySpec& a) {
        return !a.accumulate && a.k >= 1 && a.k <= static_cast<uint32_t>(kRegK) && a.r >= 1 &&
               a.r <= static_cast<uint32_t>(kRegR) && a.sz > 0 && a.nstripes > 0 && a.nstripes < (1ull << 32) &&
               a.coef_stride >= a.k && !rows_shape(a);
    };
    if (x.k != y.k || !reg_shape(x) || !reg_shape(y) || jit_mode() == kJitForce) return hipErrorNotSupported;
    const ApplySpec& a = x.r >= y.r ? x : y;
    const ApplySpec& b = x.r >= y.r ? y : x;
    const PairLaunch f = g_pair_launch[a.k][a.r][b.r];
    if (!f) return hipErrorNotSupported;
    reset_signal();
    return f(a, b, stream);
}

}  // namespace zfec_hip
