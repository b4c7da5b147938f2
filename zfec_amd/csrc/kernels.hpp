// kernels.hpp -- launch interface of the GF(2^8) matrix-apply kernels.
//
// One kernel family serves both directions of the code:
//   encode: out_i = sum_j E[block_nums[i]][j] * in_j   (zfec/fec.c:487-505)
//   decode: out_r = sum_c D[r][c] * in_c                (zfec/fec.c:527-557)
// i.e. an r x k coefficient matrix applied byte-wise to k input blocks, for
// `nstripes` independent stripes that share the matrix.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace zfec_hip {

constexpr int kMaxIn = 32;       // inputs per launch of the table / small kernels (wider: XOR-accumulating passes)
constexpr int kMaxOut = 48;      // outputs per launch
constexpr int kMaxCoef = 1536;   // r*k coefficients per launch of the table kernels
constexpr int kMaxWideIn = 256;  // inputs per launch of the bit-sliced kernels (a device-side table past kMaxIn)
constexpr int kChunk = 16;       // bytes per lane per block per step (one dwordx4)
constexpr int kMinChunk = 4;     // smallest unit any kernel variant uses (launch splitting)
constexpr int kBlock = 256;      // threads per workgroup

// One matrix application, as the host describes it (not a kernel argument:
// every kernel family builds its own, sized to what it reads).
struct ApplySpec {
    const uint8_t* coef;          // r x k coefficients, row i at coef + i * coef_stride
    uint32_t coef_stride;         // >= k
    uint32_t k, r;
    const uint8_t* const* in;     // k input block bases (stripe 0), kernel-visible addresses
    uint8_t* const* out;          // r output block bases (stripe 0)
    uint64_t sz;                  // bytes per block
    uint64_t nstripes;
    uint64_t in_sstride, out_sstride;  // stripe strides added to every input / output pointer
    bool accumulate;              // out ^= result (continuation pass of a code split by input groups)
};

// Kernel argument block of the table (matapply_lds), small and run-time-data
// bit-sliced (matapply_bsg) kernels: ~2.2 KiB, k <= kMaxIn, r <= kMaxOut.
// The register kernels (k <= 4, r <= 8) take a block sized to k + r pointers
// and their tables instead (kernels.hip, RegJob).
struct alignas(16) MatJob {
    uint64_t sz;           // bytes per block
    uint64_t in_sstride;   // stripe stride added to every input pointer
    uint64_t out_sstride;  // stripe stride added to every output pointer
    uint32_t nstripes;
    uint32_t k;            // inputs in this launch
    uint32_t r;            // outputs in this launch
    uint32_t cps;          // units per stripe
    uint32_t gs_c, gs_s;   // grid stride expressed as (units, stripes): stride = gs_s*cps + gs_c
    uint32_t accumulate;   // 1: out ^= result
    uint32_t pad_;
    const uint8_t* in[kMaxIn];
    uint8_t* out[kMaxOut];
    uint8_t coef[kMaxCoef];  // r x k row-major (matapply_bsg: its walk order)
};

// Enqueue one launch on `stream` (the current device's).  Returns
// hipErrorInvalidValue for shapes no kernel accepts (the caller splits),
// hipErrorNotSupported when a wide launch (k > kMaxIn) has no kernel for its
// shape (the caller splits it into XOR-accumulating passes).
hipError_t launch_apply(const ApplySpec& a, hipStream_t stream);

// Two independent applications over the same k in ONE launch (matapply_pair):
// both register-kernel shapes (k <= 4, r <= 8, not matapply_rows' short
// blocks), the narrower one's r <= k.  hipErrorNotSupported otherwise (the
// caller launches them one at a time).  Neither may read what the other writes.
hipError_t launch_apply_pair(const ApplySpec& x, const ApplySpec& y, hipStream_t stream);

// A batched decode with a pattern per stripe (matapply_mixed<K>, k <= 4): k
// inputs and k outputs per stripe, stripe s applying the k x k matrix
// rows + ids[s] * k * k.  The ids are nstripes uint32 in host memory (ids_host:
// copied, then uploaded with the tables) or, with ids_host null, in device
// memory (ids_dev: read in place; an id >= npatterns leaves its stripe
// unwritten).  The tables (and host ids) go through pinned staging slots by a
// stream-ordered copy, so the call declines under graph capture
// (hipErrorNotSupported).  hipErrorInvalidValue for other shapes.
constexpr uint32_t kMixedMaxK = 4;
constexpr uint32_t kMixedMaxPatterns = 65536;  // patterns per call
struct MixedSpec {
    uint32_t k;
    const uint8_t* rows;  // npatterns x k x k coefficients (host memory)
    uint32_t npatterns;
    const uint32_t* ids_host;
    const uint32_t* ids_dev;
    const uint8_t* const* in;  // k input block bases (stripe 0), kernel-visible addresses
    uint8_t* const* out;       // k output block bases (stripe 0)
    uint64_t sz, nstripes;
    uint64_t in_sstride, out_sstride;
};
hipError_t launch_mixed(const MixedSpec& m, hipStream_t stream);

// A batched repair with a pattern per stripe (matrepair_mixed<K, R>, k <= 4):
// k inputs and t output rows per stripe, stripe s applying the t x k matrix
// rows + ids[s] * t * k and storing row i only where bit i of masks[ids[s]] is
// set; a row whose bit is clear is not touched.  More than 8 rows run as
// launches of at most 8 over one upload; a group of rows no pattern stores is
// skipped, and a call that stores nothing launches nothing.  Ids, staging and
// graph capture as launch_mixed.
constexpr uint32_t kRepairMaxRows = 32;
struct RepairSpec {
    uint32_t k, t;
    const uint8_t* rows;    // npatterns x t x k coefficients (host memory)
    const uint32_t* masks;  // npatterns live-row masks (host memory)
    uint32_t npatterns;
    const uint32_t* ids_host;
    const uint32_t* ids_dev;
    const uint8_t* const* in;  // k input block bases (stripe 0), kernel-visible addresses
    uint8_t* const* out;       // t output row bases (stripe 0)
    uint64_t sz, nstripes;
    uint64_t in_sstride, out_sstride;
};
hipError_t launch_repair(const RepairSpec& p, hipStream_t stream);

// The parity update of changed primaries (matupdate_reg<C, R>, any k): stripe s
// carries c input slots, slot i the delta of primary changed[s * c + i] (or its
// old and new bytes: oldb non-null), and every stored row i gets
// coefs[j * nrows + i] * delta XOR-ed in, in place; coefs column-major by
// primary: coefs[j * nrows + i] = E[block_nums[i]][j].  A slot whose number is
// not < k is not read; a row whose coefficients for the stripe's live slots are
// all zero is neither read nor written.  More than 8 rows run as launches of 8
// over one upload, each re-reading the inputs.  The numbers are nstripes x c
// uint32 in host memory (changed_host: uploaded with the records) or in device
// memory (changed_dev: read in place).  Staging and graph capture as
// launch_mixed.
constexpr uint32_t kUpdateMaxSlots = 4;
constexpr uint32_t kUpdateMaxRows = 256;
struct UpdateSpec {
    uint32_t k, nrows, c;
    const uint8_t* coefs;  // k x nrows coefficients (host memory)
    const uint32_t* changed_host;
    const uint32_t* changed_dev;
    const uint8_t* oldb;  // slot 0 of stripe 0, or null: newb holds the deltas
    const uint8_t* newb;
    uint64_t in_bstride, in_sstride;
    uint8_t* const* rows;  // nrows row bases (stripe 0), kernel-visible addresses
    uint64_t row_sstride;
    uint64_t sz, nstripes;
};
hipError_t launch_update(const UpdateSpec& p, hipStream_t stream);

// The same two calls for wider codes (4 < k <= kMaxIn, sz >= 2048,
// generic_mode() == 2): launch_mixed and launch_repair build one record per
// pattern (below) into the same staging slot and make ONE launch of the mix
// form of the run-time-data bit-sliced kernels -- matapply_bsr<RT,mix> (r <= 10,
// one wave per 2 KiB unit) or matapply_bsr<RT,lds,mix> (2 waves for r <= 20, 4
// for r <= 32, a tile of RT = ceil(r / waves) rows each).  They return
// hipErrorNotSupported, with nothing enqueued, where that launch declines
// (bsr_mix_ok false, no routine table on the device, records past
// kBsrMixMaxBytes, 2^32 - 2^24 units): the caller takes its run path.
//
// A pattern's record: the routine addresses of its r x k matrix in the
// kernels' walk order [wave][input][RT] (the first input's are the "set"
// twins, rows past a wave's tile routine 0), then one dword live-row mask,
// padded to 16 bytes.  The layout depends on (k, r) alone, so records built
// once serve any later call.  launch_bsr_mixed launches over records and ids
// already in device memory; it touches nothing the library owns, so it may be
// captured into a graph once the routine-table probe has run on the device
// (it synchronises a stream of its own, so it does not run under capture;
// repair_records_fill below runs it).
constexpr size_t kBsrMixMaxBytes = size_t(32) << 20;  // records of one call or plan (10^4 K=20 decode patterns)
bool bsr_mix_ok(uint32_t k, uint32_t r, uint64_t sz);
size_t bsr_mix_record_bytes(uint32_t k, uint32_t r);
// npatterns records into dst (host memory) from rows (npatterns x r x k
// coefficients) and masks (npatterns; null: every row live); base: the routine
// table's address on the device
bool bsr_mix_fill_records(void* dst, const uint8_t* rows, const uint32_t* masks, size_t npatterns, uint32_t k,
                          uint32_t r, uint64_t base);
struct BsrMixSpec {
    uint32_t k, r;
    uint32_t npatterns;
    const void* records;       // device: npatterns x bsr_mix_record_bytes(k, r)
    const uint32_t* ids;       // device: nstripes pattern ids
    const uint8_t* const* in;  // k input block bases (stripe 0), device memory
    uint8_t* const* out;       // r output row bases (stripe 0)
    uint64_t sz, nstripes;
    uint64_t in_sstride, out_sstride;
};
hipError_t launch_bsr_mixed(const BsrMixSpec& m, hipStream_t stream);

// Records built once and launched over many times (fec_repair_plan_new,
// fec_repair_batch_planned).  repair_records_bytes: the bytes of npatterns
// records of a (k, t) repair -- matrepair_mixed's layout for k <= 4, the mix
// form's for 4 < k <= kMaxIn; 0 for other shapes.  repair_records_fill writes
// them into host memory (hipErrorNotSupported where the current device has no
// routine table; not under capture).  launch_repair_records launches over such
// records in device memory: `p` as for launch_repair with rows ignored and
// masks the patterns' live-row masks (host memory).  With ids in device memory
// it stages nothing, so it may be captured into a graph; host-side ids go
// through a staging slot (hipErrorNotSupported under capture).  It also returns
// hipErrorNotSupported, with nothing enqueued, where launch_bsr_mixed declines.
size_t repair_records_bytes(uint32_t k, uint32_t t, size_t npatterns);
hipError_t repair_records_fill(void* dst, const uint8_t* rows, const uint32_t* masks, size_t npatterns, uint32_t k,
                               uint32_t t);
hipError_t launch_repair_records(const RepairSpec& p, const void* records, hipStream_t stream);

// Parity verification (fec_verify_batch): nothing is written but mismatch bits.
// Bit (bit0 + i) % 32 of mismatch[s * words + (bit0 + i) / 32] is OR-ed in
// (relaxed, device scope) when row i of stripe s differs in at least one byte;
// clean data performs no store and no atomic.  The words are cleared by the
// caller, in stream order, before the launch.  mismatch is device memory.
//
// launch_verify (matverify_reg<K, R>, k <= 4, r <= 8): row i is the r x k
// matrix `coef` applied to the k basis blocks, compared with the stored check
// block chk[i]; basis and checks share the stripe stride.
// launch_rows_differ (rows_differ, r <= kMaxOut): row i of a against row i of b.
// hipErrorInvalidValue for other shapes.
struct VerifySpec {
    const uint8_t* coef;  // r x k coefficients, row i at coef + i * coef_stride
    uint32_t coef_stride;
    uint32_t k, r;
    const uint8_t* const* in;   // k basis block bases (stripe 0), kernel-visible addresses
    const uint8_t* const* chk;  // r stored check block bases (stripe 0)
    uint64_t sz, nstripes, sstride;
    uint32_t* mismatch;
    uint32_t words, bit0;
};
hipError_t launch_verify(const VerifySpec& v, hipStream_t stream);

// launch_verify_bsr (matverify_bsr<RT>, <RT,lds>, <RT,lds,tbl>; 4 < k <= 32,
// r <= kVerifyBsrRows, sz >= 2048, generic_mode() == 2): the run-time-data
// bit-sliced kernels' walk over the k basis blocks with the r computed rows
// kept as bit-planes in registers and compared with the stored check blocks in
// place -- every block read once, no scratch, nothing stored to block memory.
// The kernel form, tiles and routine-address table are launch_apply's for the
// same (k, r, units).  hipErrorNotSupported wherever that path would decline
// (shape, no routine table on the device, a table past its cache slot, 2^32
// units): the caller takes the two-step path.  verify_bsr_ok: the shape part
// of that decision (no device needed); r past kVerifyBsrRows stands for a
// first launch of kVerifyBsrRows rows.
constexpr uint32_t kVerifyBsrRows = 40;
bool verify_bsr_ok(uint32_t k, uint32_t r, uint64_t sz);
hipError_t launch_verify_bsr(const VerifySpec& v, hipStream_t stream);

struct DifferSpec {
    uint32_t r;
    const uint8_t* const* a;  // r row bases (stripe 0)
    const uint8_t* const* b;
    uint64_t sz, nstripes, a_sstride, b_sstride;
    uint32_t* mismatch;
    uint32_t words, bit0;
};
hipError_t launch_rows_differ(const DifferSpec& d, hipStream_t stream);

// Single-block error location (fec_locate_batch).  Every stripe has `words`
// working words in device memory, cleared by the caller in stream order:
// mismatch bit i at bit index i (as above), excluded bit j of basis slot j at
// bit index xbit + j, OR-ed in when the hypothesis "only basis slot j is
// corrupt" is refuted at some byte.  q: Q[i][j] = P[i][j] / P[0][j] for
// i = 1..c-1, (c-1) x k row-major.
//
// launch_locate (matlocate_reg<K, R>, k <= 4, 2 <= r <= 8): all r = c checks in
// one launch; `v` as for launch_verify with bit0 = 0.
// locate_tables_upload: the k*(c-1) tables of q into device memory through the
// thread's staging ring, by one stream-ordered copy; locate_tables_release
// after the last launch that reads them (it records the slot's event).
// launch_rows_locate (rows_locate): rows [d.bit0, d.bit0 + d.r) of the c checks,
// a0 / b0 row 0's pair (stripe 0 of the launch, as a and b).
// launch_locate_finish (locate_finish): the words of nstripes stripes into one
// verdict dword each; it leaves matapply_last_kernel() as it was.
struct LocateTables {
    const uint32_t* dev = nullptr;
    void* slot = nullptr;
};
hipError_t launch_locate(const VerifySpec& v, const uint8_t* q, uint32_t xbit, hipStream_t stream);
hipError_t locate_tables_upload(const uint8_t* q, uint32_t k, uint32_t c, hipStream_t stream, LocateTables* out);
void locate_tables_release(const LocateTables& t, hipStream_t stream);
hipError_t launch_rows_locate(const DifferSpec& d, const uint8_t* a0, const uint8_t* b0, uint32_t k, uint32_t xbit,
                              const uint32_t* qtab_dev, hipStream_t stream);
hipError_t launch_locate_finish(const uint32_t* bits, uint32_t words, uint32_t k, uint32_t c, uint64_t nstripes,
                                uint32_t* culprit, hipStream_t stream);

// In-place correction (fec_correct_batch) over the verdict words
// launch_locate_finish wrote, in device memory: a stripe whose verdict h is
// below nb has slot h (at blocks + h * bstride) rewritten as row h of `rows`
// (nb x k coefficients, host memory) applied to slots 0..k-1, slot k taking
// slot h's place when h < k; every other stripe costs one scalar load per wave
// and is neither read nor written.  matcorrect_reg<k> for k <= 4, rows_correct
// past that.  The nb x k tables go through the thread's staging ring by one
// stream-ordered copy, the slot's event recorded after the last launch, so the
// call declines under graph capture (hipErrorNotSupported).
struct CorrectSpec {
    uint32_t k, nb;
    const uint8_t* rows;  // nb x k coefficients (host memory)
    uint8_t* blocks;      // slot 0 of stripe 0, a kernel-visible address
    uint64_t bstride, sstride;
    uint64_t sz, nstripes;
    const uint32_t* verdict;  // nstripes words, device memory
};
hipError_t launch_correct(const CorrectSpec& p, hipStream_t stream);

// Pair location and correction (fec_locate2_batch, fec_correct2_batch) over the
// stripes the single-block rules call MANY, for c >= 4 checks and nb = k + c <=
// 32 slots.  Pair (a, b), a < b, has index a*nb - a(a+1)/2 + (b - a - 1).
//
// launch_locate2_finish (locate2_finish): launch_locate_finish's verdicts into
// culprit[0..nstripes) and NONE into culprit[nstripes..2 nstripes).  With list
// and pairbits (both or neither; device memory the library owns, 1 + nstripes
// and nstripes * pairs_words(nb) words; list[0] cleared by the caller in
// stream order) every MANY stripe takes the next list entry and has the
// entry's pair words cleared.
//
// launch_pairs: one staged upload (so hipErrorNotSupported under capture), then
// pairs_locate (refuted pair bits OR-ed into the entries' words), pairs_finish
// (an entry with exactly one pair left gets (a, b) in the two planes) and, with
// sources / crows, pairs_correct (slots a and b of such a stripe rewritten in
// place).  All three run over fixed grids and do nothing on an empty list.
//   pivots: per pair 2 + 3 (c - 2) bytes: r0, r1, then (i, alpha, beta) for
//     every other row i: s_i ^ alpha . s_r0 ^ beta . s_r1 vanishes exactly on
//     span(p_a, p_b);
//   sources, crows: per pair the k source slots and the 2 x k coefficients
//     that yield slots a and b from them (fec_correct2_rows).
constexpr bool pairs_shape_ok(uint32_t k, uint32_t c) { return k >= 1 && c >= 4 && k + c <= 32; }
constexpr uint32_t pairs_words(uint32_t nb) { return (nb * (nb - 1) / 2 + 31) / 32; }
struct PairsSpec {
    uint32_t k, c;
    const uint8_t* P;         // c x k (host memory, as everything down to crows)
    const uint8_t* pivots;
    const uint32_t* sources;  // null: locate only
    const uint8_t* crows;
    uint8_t* blocks;          // slot 0 of stripe 0, a kernel-visible address
    uint64_t bstride, sstride;
    uint64_t sz, nstripes;
    const uint32_t* list;
    uint32_t* pairbits;
    uint32_t* culprit;   // the two planes, device memory
    uint64_t plane = 0;  // words from plane 0 to plane 1; 0: nstripes
};
// `plane`: words from plane 0 to plane 1, 0 for nstripes.  A run of a ragged
// call writes into the planes of the whole call, which lie further apart.
hipError_t launch_locate2_finish(const uint32_t* bits, uint32_t words, uint32_t k, uint32_t c, uint64_t nstripes,
                                 uint32_t* culprit, uint32_t* list, uint32_t* pairbits, hipStream_t stream,
                                 uint64_t plane = 0);
hipError_t launch_pairs(const PairsSpec& p, hipStream_t stream);

// The pair pass of a batch whose stripes each have their own size
// (pairs_locate_ragged, pairs_finish, pairs_correct_ragged;
// fec_locate2_batch_ragged / fec_correct2_batch_ragged), over the list and
// the planes launch_locate2_finish wrote after a ragged location.  sizes and
// off are device memory: what the location staged (RaggedScrubStaged) or the
// caller's arrays.  Slot j of listed stripe s is at blocks + off[s] + j * B,
// B = bstride or sizes[s] when that is 0; each kernel reads and writes a
// stripe only where it fits `bytes` by its own test over all k + c slots.
// Records, upload, fixed grids and the empty list as launch_pairs; the planes
// are nstripes words apart.
struct PairsRaggedSpec {
    uint32_t k, c;
    const uint8_t* P;         // host memory, as everything down to crows (PairsSpec)
    const uint8_t* pivots;
    const uint32_t* sources;  // null: locate only
    const uint8_t* crows;
    uint8_t* blocks;          // the arena, a kernel-visible address
    uint64_t bytes, bstride;
    const uint64_t *sizes, *off;  // nstripes each, device memory
    uint64_t nstripes;
    const uint32_t* list;
    uint32_t* pairbits;
    uint32_t* culprit;  // the two planes, device memory
};
hipError_t launch_pairs_ragged(const PairsRaggedSpec& p, hipStream_t stream);

// A batched encode or decode whose stripes each have their own size
// (matapply_ragged<K, R>, k <= 4; fec_encode_batch_ragged / fec_decode_batch_ragged).
// Stripe s has blocks of sizes[s] bytes: input j at in + in_off[s] + j * B, output
// row i at out + out_off[s] + i * B', with B = in_bstride, or sizes[s] when that
// is 0 (packed objects), and B' from out_bstride likewise.  All stripes share
// the r x k matrix `coef`; more than 8 rows run as row groups of at most 8 over
// one staging.  A stripe is read and written only where it FITS both arenas:
// off + (rows - 1) * B + size <= bytes (ragged_fits), tested by the kernel per
// stripe; zero-size stripes are neither read nor written.
//
// A unit is one wave step, 64 lanes x kChunk bytes of every block: stripe s has
// ragged_units_of(sizes[s]) of them, and ustart (ragged_units) is their
// exclusive prefix sum.  With desc_host the three arrays are host memory: the
// host computes ustart and uploads all four arrays by one staged copy.
// Otherwise they are device memory, read where they are, and ragged_scan
// writes ustart into the staging slot's device half in stream order; there a
// size that exceeds either arena counts no units.  Both forms use a staging
// slot, so the call declines under graph capture (hipErrorNotSupported).
// hipErrorInvalidValue for other shapes (k > 4: the caller cuts runs).
constexpr uint32_t kRaggedUnit = 64 * kChunk;
__host__ __device__ inline uint64_t ragged_units_of(uint64_t sz) {
    return sz / kRaggedUnit + (sz % kRaggedUnit != 0);
}
// ustart[0 .. n] from sizes[0 .. n); returns the total
inline uint64_t ragged_units(const uint64_t* sizes, uint64_t n, uint64_t* ustart) {
    uint64_t t = 0;
    for (uint64_t s = 0; s < n; ++s) {
        ustart[s] = t;
        t += ragged_units_of(sizes[s]);
    }
    ustart[n] = t;
    return t;
}
// off + (rows - 1) * stride + sz <= bytes, evaluated without wrapping (rows <= 2^32)
__host__ __device__ inline bool ragged_fits(uint64_t off, uint64_t stride, uint32_t rows, uint64_t sz,
                                            uint64_t bytes) {
    if (rows == 0) return true;  // nothing is read or written on this side
    if (sz > bytes || off > bytes - sz) return false;
    if (rows == 1) return true;
    const uint64_t room = bytes - sz - off, m = rows - 1;
    if (stride > room) return false;
    const uint64_t hi = (stride >> 32) * m + (((stride & 0xFFFFFFFFull) * m) >> 32);  // bits 32.. of the product
    return (hi >> 32) == 0 && stride * m <= room;
}
struct RaggedSpec {
    uint32_t k, r;
    const uint8_t* coef;  // r x k coefficients, row-major (host memory)
    const uint8_t* in;    // the two arenas, kernel-visible addresses
    uint8_t* out;
    uint64_t in_bytes, out_bytes;
    uint64_t in_bstride, out_bstride;
    const uint64_t *sizes, *in_off, *out_off;  // nstripes each
    bool desc_host;
    uint64_t nstripes;
};
hipError_t launch_ragged(const RaggedSpec& g, hipStream_t stream);

// The scrub of such a batch (matverify_ragged<K, R> / matlocate_ragged<K, R>,
// k <= 4; fec_verify_batch_ragged / fec_locate_batch_ragged).  Stripe s holds
// k + c blocks of sizes[s] bytes, slot j at src + off[s] + j * B with B =
// bstride, or sizes[s] when that is 0; P is the c x k matrix of the checks.
// Q null: a verify; bit i of the stripe's `words` words at bits + s * words is
// OR-ed in when check i differs, more than 8 checks as row groups of 8 over
// one staging.  Q set ((c-1) x k, 2 <= c <= 8): a location; mismatch bits from
// bit 0 and excluded bits from bit xbit of the stripe's working words, for
// launch_locate_finish.  The words are device memory the caller cleared in
// stream order.  Bits are accumulated per (wave, stripe) and OR-ed out once,
// only where nonzero.  A stripe is read only where it fits the arena; an empty
// or unfit one contributes no bit.  Descriptors, units and staging as
// launch_ragged (ragged_scan with maxsz = bytes); hipErrorNotSupported under
// capture, hipErrorInvalidValue for other shapes.
//
// launch_ragged_unfit (ragged_unfit): for descriptor arrays in device memory,
// one lane per stripe marks every nonempty stripe that does not fit: all c
// check bits of its ceil(c / 32) words at out + s * words, or with c == 0 the
// verdict FEC_LOCATE_UNFIT at out + s.  Plain stores; it stages nothing and
// leaves matapply_last_kernel() as it was.
//
// keep (may be null): where a correction follows the location, the staged
// descriptors stay valid past the call -- ustart, sizes and offsets in device
// memory, and the units that sized the grid -- until ragged_scrub_release,
// which records the slot's event after the last launch that reads them.  It is
// left with a null slot where nothing was launched (every stripe empty).
struct RaggedScrubStaged {
    void* slot = nullptr;
    const uint64_t *ustart = nullptr, *sizes = nullptr, *off = nullptr;
    uint64_t units = 0;
};
struct RaggedScrubSpec {
    uint32_t k, c;
    const uint8_t* P;    // c x k coefficients, row-major (host memory)
    const uint8_t* Q;    // (c-1) x k, or null: verify
    const uint8_t* src;  // the arena, a kernel-visible address
    uint64_t bytes, bstride;
    const uint64_t *sizes, *off;  // nstripes each
    bool desc_host;
    uint64_t nstripes;
    uint32_t* bits;
    uint32_t words, xbit;
    RaggedScrubStaged* keep = nullptr;
};
hipError_t launch_ragged_scrub(const RaggedScrubSpec& p, hipStream_t stream);
hipError_t launch_ragged_unfit(const uint64_t* sizes, const uint64_t* off, uint64_t nstripes, uint32_t slots,
                               uint64_t bstride, uint64_t bytes, uint32_t c, uint32_t* out, hipStream_t stream);
void ragged_scrub_release(const RaggedScrubStaged& t, hipStream_t stream);

// The in-place correction of such a batch (matcorrect_ragged<K>, k <= 4;
// fec_correct_batch_ragged) over the verdict words launch_locate_finish and
// launch_ragged_unfit wrote, in device memory, and the descriptors a location
// with `keep` staged: a stripe whose verdict h is below nb, and which fits the
// arena by the kernel's own test over all nb slots, has the sizes[s] bytes of
// slot h rewritten as row h of `rows` (nb x k, host memory) applied to slots
// 0..k-1, slot k taking slot h's place when h < k.  Every other stripe costs
// scalar loads and is neither read nor written.  The tables go through a
// staging slot of their own (hipErrorNotSupported under capture).  The caller
// releases `staged` afterwards.
struct RaggedCorrectSpec {
    uint32_t k, nb;
    const uint8_t* rows;  // nb x k coefficients (host memory)
    uint8_t* blocks;      // the arena, a kernel-visible address
    uint64_t bytes, bstride;
    uint64_t nstripes;
    const uint32_t* verdict;  // nstripes words, device memory
    RaggedScrubStaged staged;
};
hipError_t launch_ragged_correct(const RaggedCorrectSpec& p, hipStream_t stream);

// A batched repair whose stripes each have their own size and their own
// pattern (matrepair_ragged<K, R>, k <= 4; fec_repair_batch_ragged): the
// arenas, descriptors, fit rule and units of launch_ragged, the patterns of
// launch_repair.  Stripe s uses pattern ids[s]; with neither ids_host nor
// ids_dev (npatterns == 1) every stripe uses pattern 0.  Row i of a stripe is
// stored at out + out_off[s] + i * B' only where bit i of its pattern's mask
// is set; the fit test covers all t rows.  A stripe that does not fit, or
// whose id is >= npatterns, is neither read nor written.  More than 8 targets
// run as row groups of 8 over one staging; a group no pattern uses is skipped,
// and a call no pattern of which has a live row launches nothing.  One staging
// slot holds records, host-side ids and host-side descriptors (one copy), or
// records, host-side ids and ragged_scan's ustart; hipErrorNotSupported under
// capture, hipErrorInvalidValue for other shapes (k > 4: the caller cuts runs).
struct RaggedRepairSpec {
    uint32_t k, t;
    const uint8_t* rows;     // npatterns x t x k coefficients (host memory)
    const uint32_t* masks;   // npatterns live-row masks (host memory)
    uint32_t npatterns;
    const uint32_t* ids_host;  // nstripes ids in host memory, or
    const uint32_t* ids_dev;   // in device memory, or neither
    const uint8_t* in;         // the two arenas, kernel-visible addresses
    uint8_t* out;
    uint64_t in_bytes, out_bytes;
    uint64_t in_bstride, out_bstride;
    const uint64_t *sizes, *in_off, *out_off;  // nstripes each
    bool desc_host;
    uint64_t nstripes;
};
hipError_t launch_ragged_repair(const RaggedRepairSpec& p, hipStream_t stream);

// The parity update of such a batch (matupdate_ragged<C, R>, ANY k;
// fec_update_batch_ragged): the arithmetic, records and numbers of
// launch_update, the arenas, descriptors, fit rule and units of launch_ragged.
// Input slot i of stripe s is at newb + in_off[s] + i * B (and at the same
// offset in oldb, a second arena of in_bytes, where that is non-null), stored
// row i at rows + row_off[s] + i * B'; the fit test covers c slots and all
// nrows rows.  A stripe that does not fit, or none of whose numbers is < k, is
// neither read nor written; a row is read and written only where a live slot's
// coefficient for it is not zero.  More than 8 rows run as row groups of 8
// over one staging, each re-reading the inputs.  One staging slot holds the
// records, host-side numbers and host-side descriptors (one copy), or the
// records, host-side numbers and ragged_scan's ustart; hipErrorNotSupported
// under capture.  Every code takes this one path: nothing is cut into runs and
// nothing synchronises.
struct RaggedUpdateSpec {
    uint32_t k, nrows, c;
    const uint8_t* coefs;  // k x nrows coefficients, as UpdateSpec's (host memory)
    const uint32_t* changed_host;  // nstripes x c numbers in host memory, or
    const uint32_t* changed_dev;   // in device memory
    const uint8_t* oldb;           // the arenas, kernel-visible addresses; oldb may be null
    const uint8_t* newb;
    uint8_t* rows;
    uint64_t in_bytes, row_bytes;
    uint64_t in_bstride, row_bstride;
    const uint64_t *sizes, *in_off, *row_off;  // nstripes each
    bool desc_host;
    uint64_t nstripes;
};
hipError_t launch_ragged_update(const RaggedUpdateSpec& p, hipStream_t stream);

// Whether `stream` is being captured into a HIP graph.  The table forms (a
// device-side table the host fills and reuses at enqueue time) decline then:
// a captured graph would replay copies from host slots rewritten since, or
// read a cached device table whose upload was only recorded.  launch_apply
// falls back to kernels whose whole description travels in their arguments;
// wide launches (k > kMaxIn) are split into passes by the caller.
bool stream_capturing(hipStream_t stream);

// Whether launch_apply takes all k > kMaxIn inputs of a launch of r <= kMaxOut
// rows, sz-byte blocks and nstripes stripes in one pass (bit-sliced kernels).
bool wide_launch_ok(uint32_t k, uint32_t r, uint64_t sz, uint64_t nstripes);

// Ask the calling thread's next launch_apply to have its kernel publish `seq`
// at flag_dev (pinned host memory) when it has finished -- honoured only by
// the register kernels in a one-workgroup launch (a stripe of at most 4 KiB
// per block); matapply_signal_used() says whether it was.
void matapply_request_signal(uint32_t* flag_dev, uint32_t seq);
bool matapply_signal_used();

// The synchronous small call's launch (fec_abi.cpp run_single, every block in
// the thread's pinned bounce buffer): k <= 4, r <= 8, one stripe of sz bytes,
// sz a multiple of 16 and at most 4096 (whole 16-byte units, one workgroup).
// matapply_one publishes `seq` at flag_dev (pinned host memory, may be null)
// when it has finished.  host_in (may be null): the k input blocks of host_sz
// bytes each in host memory; where they fit (k x sz rounded to 16 bytes at
// most 4,352 bytes) they are copied into the kernel's argument block and
// a.in is not read.  hipErrorInvalidValue for other shapes.
constexpr uint32_t kOneInlineBytes = 4352;  // inline input capacity of matapply_one's argument block
// Whether k host inputs of host_sz bytes, padded to ksz (a whole number of
// 16-byte units), go inside matapply_one's argument block: the one test both
// run_single (which then skips the copy into the bounce buffer) and
// launch_one use.
constexpr bool one_inline_fits(uint32_t k, uint64_t ksz, uint64_t host_sz) {
    return host_sz <= ksz && ksz % 16 == 0 && uint64_t(k) * ksz <= kOneInlineBytes;
}
hipError_t launch_one(const ApplySpec& a, hipStream_t stream, uint32_t* flag_dev, uint32_t seq,
                      const uint8_t* const* host_in = nullptr, uint64_t host_sz = 0);

// Name of the table-kernel variant launch_apply uses for (k, r) when no
// run-time specialised kernel applies (for tests / profiling).
const char* matapply_variant_name(uint32_t k, uint32_t r, bool accumulate);

// Name of the kernel the calling thread launched last (table variant,
// run-time-data bit-sliced kernel matapply_bsg, or bit-sliced JIT kernel,
// bitslice.hpp).
const char* matapply_last_kernel();

// The bit-sliced kernels with the coefficients as run-time data, for wide-code
// launches that no specialised JIT kernel serves: 2 = matapply_bsr (default;
// matapply_bsg for the few shapes it does not take); 1 = matapply_bsg only;
// 0 = off (the table kernels serve).  Env ZFEC_HIP_GENERIC=0/1/2 starts
// in that mode.
int generic_mode();
void set_generic_mode(int mode);

}  // namespace zfec_hip
