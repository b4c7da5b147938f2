/*
 * zfec_hip.h -- C-ABI of libzfec_hip.so, the MI355X (gfx950) erasure-coding engine.
 *
 * Part 1 is a drop-in for zfec's own C interface (/root/reference/zfec/fec.h):
 * same names, same argument meaning, same ownership rules, bit-identical
 * results.  A program (or FFI binding: zfec/_fecmodule.c, haskell/Codec/FEC.hs)
 * written against fec.h links against this library unchanged.  Buffers may be
 * host memory or device memory (hipMalloc / torch CUDA tensors); the library
 * detects which per pointer.  The GF(2^8) multiply-accumulate always runs in
 * HIP kernels on the GPU -- there is no CPU compute path.
 *
 * Part 2 adds what a GPU caller needs: status codes instead of assert(),
 * stream-ordered asynchronous variants, and batched strided entry points
 * that encode/decode many independent stripes in one launch.
 *
 * Plain C types only (stream handles are passed as void*, i.e. hipStream_t).
 */
#ifndef ZFEC_HIP_H
#define ZFEC_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* zfec/fec.h:9 */
typedef unsigned char gf;

/* zfec/fec.h:11-15.  The first three fields keep the reference layout (C callers
 * may read k and n); `priv` is library-private and follows them. */
typedef struct {
    unsigned long magic;
    unsigned short k, n; /* parameters of the code */
    gf* enc_matrix;      /* n x k row-major systematic encoding matrix (host memory) */
    void* priv;
} fec_t;

/* ---------------------------------------------------------------------------
 * Part 1: zfec/fec.h drop-in
 * ------------------------------------------------------------------------- */

/* Replaces zfec/fec.h:33 / fec.c:406-413.  Builds the GF(2^8) tables.  Unlike
 * the reference it is idempotent and thread-safe (std::call_once). */
void fec_init(void);

/* Replaces zfec/fec.h:39 / fec.c:430-479.  Returns NULL (and sets the
 * thread-local status) on invalid parameters (k < 1, m > 256, k > m) instead
 * of assert(); returns NULL if fec_init() was never called, like the reference
 * (fec.c:442-444). */
fec_t* fec_new(unsigned short k, unsigned short m);

/* Replaces zfec/fec.h:40 / fec.c:423-428. */
void fec_free(fec_t* p);

/* Replaces zfec/fec.h:49 / fec.c:487-505.  fecs[i] receives block
 * block_nums[i] (sz bytes) for i < num_block_nums.  Synchronous: the outputs
 * are complete when it returns.  Errors (block number >= n, HIP failure) set
 * the thread-local status and leave outputs unspecified; they never abort.
 * Extension: a block number < k yields a copy of that primary block (the
 * reference asserts, fec.c:498). */
void fec_encode(const fec_t* code, const gf* const* src, gf* const* fecs,
                const unsigned* block_nums, size_t num_block_nums, size_t sz);

/* Replaces zfec/fec.h:57 / fec.c:527-557.  inpkts[i] holds block index[i];
 * a present primary block i must sit at slot i.  outpkts receives the missing
 * primaries in ascending order.  Synchronous. */
void fec_decode(const fec_t* code, const gf* const* inpkts, gf* const* outpkts,
                const unsigned* index, size_t sz);

/* Exported by the reference too (fec.c:512-525, fec.c:341-394). */
void build_decode_matrix_into_space(const fec_t* code, const unsigned* index, const unsigned k, gf* matrix);
void _invert_vdm(gf* src, unsigned k);

/* ---------------------------------------------------------------------------
 * Part 2: extensions
 * ------------------------------------------------------------------------- */

enum {
    FEC_OK = 0,
    FEC_EINVAL = 1,     /* bad argument (k/m range, block number, duplicate, NULL) */
    FEC_ENODEV = 2,     /* no usable GPU */
    FEC_EHIP = 3,       /* a HIP runtime call failed */
    FEC_ENOMEM = 4,     /* allocation failed */
    FEC_ESINGULAR = 5,  /* decode matrix singular (duplicate block numbers) */
    FEC_EUNINIT = 6     /* fec_init() not called */
};

#define FEC_FLAG_ASYNC 1u          /* do not synchronize; all buffers device or page-locked host memory */
#define FEC_FLAG_LIBRARY_STREAM 2u /* ignore `stream`; use the library's per-thread stream */
#define FEC_FLAG_ALL_PRIMARIES 4u  /* decode: output all k primaries in order (present ones copied),
                                      not only the missing ones: the output is the stripe itself */
#define FEC_FLAG_HOST_MEMORY 8u    /* every block is host memory (pageable or page-locked): skip the
                                      per-pointer device queries (small calls from Python bytes) */
#define FEC_FLAG_ROW_PADDING 16u   /* batched calls: every block row may be read (inputs) and written
                                      (outputs) up to the next multiple of 128 bytes past its end, so
                                      each row ends on a whole cache line; output bytes past sz are
                                      then unspecified.  Used only when the block and stripe strides
                                      leave that much room; otherwise ignored */
#define FEC_FLAG_NO_POPULATE 32u   /* accepted and ignored (round 2's page-locking host path, which
                                      pre-faulted outputs, was removed: the staged path never locks) */

/* Status of the last library call made by this thread, and its message. */
int fec_last_status(void);
const char* fec_last_error_message(void);

/* fec_encode / fec_decode returning a status, on a caller-chosen HIP stream.
 * `stream` follows HIP's convention: NULL is the null (legacy default) stream,
 * which is what torch's default stream hands out.  FEC_FLAG_LIBRARY_STREAM
 * selects the library's own per-thread non-blocking stream instead (what the
 * synchronous fec_encode / fec_decode use).  With FEC_FLAG_ASYNC and device or
 * page-locked host buffers the call only enqueues work on the stream.
 *
 * Host buffers: page-locked ones (fec_host_alloc, hipHostMalloc,
 * hipHostRegister) are read and written by the kernel in place over PCIe;
 * large pageable ones are copied through pinned staging slots by the
 * library's host threads, chunk by chunk, overlapped with the kernels; small
 * pageable ones go through a bounce buffer.  Calls with pageable host buffers
 * are synchronous whatever the flags. */
int fec_encode_ex(const fec_t* code, const gf* const* src, gf* const* fecs,
                  const unsigned* block_nums, size_t num_block_nums, size_t sz,
                  void* stream, unsigned flags);
int fec_decode_ex(const fec_t* code, const gf* const* inpkts, gf* const* outpkts,
                  const unsigned* index, size_t sz, void* stream, unsigned flags);

/* Batched encode of nstripes independent stripes in one launch (device memory
 * on one device, or page-locked host memory).  Pageable host memory on either
 * side is accepted too: it is staged through pinned slots in groups of stripes
 * by the library's host threads (only the rows are written; the call is then
 * synchronous and FEC_FLAG_ROW_PADDING does not apply).  Block j of stripe s is read from src + s*src_stripe_stride +
 * j*src_block_stride; output i of stripe s (block block_nums[i]) is written to
 * dst + s*dst_stripe_stride + i*dst_block_stride.  Packed [stripe][block][sz]
 * layouts use block_stride = sz, stripe_stride = k*sz (input) / num*sz (output).
 * Block-major layouts (block j of every stripe back to back: stripe_stride = sz
 * on both sides, block_stride >= nstripes*sz) run as one stripe of nstripes*sz
 * bytes, the fastest shape for many small objects. */
int fec_encode_batch(const fec_t* code,
                     const gf* src, size_t src_block_stride, size_t src_stripe_stride,
                     gf* dst, size_t dst_block_stride, size_t dst_stripe_stride,
                     const unsigned* block_nums, size_t num_block_nums, size_t sz,
                     size_t nstripes, void* stream, unsigned flags);

/* Batched decode: every stripe received the same block numbers (index[slot],
 * primaries at their own slot as in fec_decode).  Slot j of stripe s at
 * src + s*src_stripe_stride + j*src_block_stride; the recovered primaries
 * (ascending) at dst + s*dst_stripe_stride + i*dst_block_stride. */
int fec_decode_batch(const fec_t* code,
                     const gf* src, size_t src_block_stride, size_t src_stripe_stride,
                     gf* dst, size_t dst_block_stride, size_t dst_stripe_stride,
                     const unsigned* index, size_t sz, size_t nstripes,
                     void* stream, unsigned flags);

/* Ragged batches: batched encode and decode whose stripes each have their own
 * size (a store's objects do not share a length; a file cut into segments ends
 * in a short one), in one launch.
 *
 * Stripe s has blocks of sizes[s] bytes; 0 is allowed, and such a stripe is
 * neither read nor written.  Input block j of stripe s starts at
 * src + src_offsets[s] + j*B, with B = src_block_stride when that is nonzero and
 * B = sizes[s] otherwise: the packed object [block 0 | block 1 | ... | block
 * k-1], which is what an easyfec-style object whose length is a multiple of k
 * already is.  Output row i of stripe s starts at dst + dst_offsets[s] + i*B',
 * B' from dst_block_stride / sizes[s] in the same way.  A nonzero fixed stride
 * describes block-major arenas: block j of every stripe lies in arena j, and
 * the offsets are a prefix sum of the sizes.  Offsets are arbitrary bytes: no
 * alignment, no ordering.  Outputs must not overlap each other or the inputs.
 *
 * fec_encode_batch_ragged writes the blocks block_nums[0..num_block_nums) as
 * fec_encode_batch does (a number below k copies that primary);
 * fec_decode_batch_ragged takes fec_decode_batch's index (primary i at slot i)
 * and writes the missing primaries in ascending order, or with
 * FEC_FLAG_ALL_PRIMARIES all k.  The bytes are those of fec_encode_batch /
 * fec_decode_batch called once per stripe with nstripes = 1.
 *
 * sizes, src_offsets and dst_offsets are three arrays of nstripes 8-byte words
 * (8-byte aligned), all three in host memory or all three in device memory on
 * the blocks' device; a mix returns FEC_EINVAL.  Host arrays are copied when the
 * call is made and may be reused when it returns; device arrays are read where
 * they are, in stream order, and nothing synchronises the stream.
 *
 * src_bytes and dst_bytes are the extents of the two arenas.  A stripe with
 * sizes[s] > 0 FITS when offset + (rows - 1)*B + sizes[s] <= bytes on both sides
 * (rows = k for src, the output rows for dst), evaluated without wrapping.
 * With host arrays a stripe that does not fit is FEC_EINVAL, the message naming
 * the stripe and the side.  Device arrays the host cannot look at: the kernel
 * makes the same test per stripe, a stripe that does not fit is neither read
 * nor written, and no error is reported (the rule an id >= npatterns follows
 * in fec_decode_batch_mixed) -- a wrong device-side descriptor leaves bytes
 * untouched instead of causing a wild access.
 *
 * src and dst are device memory on one device, or page-locked host memory;
 * pageable host memory returns FEC_EINVAL (this call does not stage).
 * FEC_FLAG_ASYNC and FEC_FLAG_LIBRARY_STREAM as in fec_decode_batch;
 * FEC_FLAG_ROW_PADDING is accepted and ignored.  While the stream is being
 * captured into a graph the call returns FEC_EINVAL: it stages per call through
 * slots the library reuses.
 *
 * Checked before any GPU work, in this order, each FEC_EINVAL with a message:
 * an invalid fec_t; a NULL src, dst, sizes, src_offsets, dst_offsets or
 * block_nums / index; num_block_nums == 0 or a block number >= n (decode: the
 * checks of fec_decode_batch); nstripes >= 2^32; descriptor arrays of mixed
 * memory kinds; with host arrays a stripe that does not fit.  Then FEC_ENODEV
 * when no GPU is visible.  nstripes == 0 returns FEC_OK, and so does a batch
 * whose sizes are all zero, which with host arrays launches nothing.
 *
 * k <= 4 is one launch of matapply_ragged<k,r> per 8 output rows: every wave
 * walks a contiguous range of 1 KiB wave steps ("units", fec_ragged_units) and
 * reads each stripe's size and offsets by scalar loads; with device arrays a
 * short scan kernel (ragged_scan) first writes the units' prefix sum into
 * memory the library owns.  Wider codes are cut into runs of consecutive
 * stripes of one size whose two offsets each advance by a constant, each run
 * one fec_encode_batch / fec_decode_batch-style launch (at worst one per
 * stripe); on that path device-side arrays are first copied to the host, which
 * SYNCHRONISES the stream, and stripes that do not fit are skipped there too. */
int fec_encode_batch_ragged(const fec_t* code,
                            const gf* src, size_t src_bytes, size_t src_block_stride,
                            const unsigned long long* src_offsets,
                            gf* dst, size_t dst_bytes, size_t dst_block_stride,
                            const unsigned long long* dst_offsets,
                            const unsigned long long* sizes,
                            const unsigned* block_nums, size_t num_block_nums,
                            size_t nstripes, void* stream, unsigned flags);
int fec_decode_batch_ragged(const fec_t* code,
                            const gf* src, size_t src_bytes, size_t src_block_stride,
                            const unsigned long long* src_offsets,
                            gf* dst, size_t dst_bytes, size_t dst_block_stride,
                            const unsigned long long* dst_offsets,
                            const unsigned long long* sizes,
                            const unsigned* index,
                            size_t nstripes, void* stream, unsigned flags);

/* Host only, no GPU: the units of a ragged batch.  Stripe s has
 * u(s) = ceil(sizes[s] / 1024) units -- one unit is one wave step, 64 lanes x
 * 16 bytes of every block -- and ustart[0..nstripes] receives their exclusive
 * prefix sum, so ustart[nstripes] is the total.  FEC_OK / FEC_EINVAL (NULL). */
int fec_ragged_units(const unsigned long long* sizes, size_t nstripes, unsigned long long* ustart);

/* Batched decode, a pattern per stripe: every stripe of the batch may have
 * received different blocks (a storage node repairing many small objects).
 * patterns: npatterns x k block numbers (host memory); pattern p says slot j of
 * a stripe holds block patterns[p*k+j].  A pattern's k numbers are distinct and
 * less than n, in ANY slot order (fec_decode's "primary i at slot i" is not
 * required).  pattern_of: nstripes pattern ids (unsigned, 4 bytes each), in host
 * OR device memory.  Output: all k primaries of every stripe in order (the stripe
 * itself, FEC_FLAG_ALL_PRIMARIES semantics: a present primary is copied), k rows
 * per stripe: primary i of stripe s at dst + s*dst_stripe_stride +
 * i*dst_block_stride.  Bit-identical to fec_decode whatever the slot order.
 *
 * src and dst are device memory on one device, or page-locked host memory;
 * pageable host memory returns FEC_EINVAL (this call does not stage).  Strides
 * as in fec_decode_batch, except that a block-major layout is walked stripe by
 * stripe (its stripes do not share a matrix, so it is not collapsed).
 * FEC_FLAG_ASYNC and FEC_FLAG_LIBRARY_STREAM as in fec_decode_batch;
 * FEC_FLAG_ROW_PADDING is accepted and ignored.
 *
 * All arguments are checked before any GPU work: a NULL argument, npatterns ==
 * 0 with stripes to decode, more than 65536 patterns, a block number >= n or a
 * duplicate in a pattern, and an id >= npatterns in a HOST-side pattern_of
 * return FEC_EINVAL with a message naming the pattern or stripe.  Ids in DEVICE
 * memory cannot be checked by the host: a stripe whose id is >= npatterns is
 * left unwritten (no table is read for it), and no error is reported.
 *
 * k <= 4 runs in one launch of matapply_mixed<k>; the per-pattern tables (and
 * host-side ids) are uploaded by a stream-ordered copy from pinned staging the
 * library owns, so pattern_of and patterns may be reused as soon as the call
 * returns.  4 < k <= 32 with sz >= 2048 and the blocks in device memory is one
 * launch too, of matapply_bsr<RT,mix> / <RT,lds,mix>: one record of routine
 * addresses per pattern goes through the same staging, a device-side
 * pattern_of is read where it is, and nothing synchronises the stream (each
 * pattern costs the host one k x k inversion per call: fec_repair_plan_new
 * builds the records once).  The remaining shapes -- k > 32, sz < 2048,
 * page-locked host blocks, more than 32 MiB of records, no routine table on the
 * device, ZFEC_HIP_MIXED_FUSED=0 -- are cut into runs of consecutive stripes with
 * one id, each run one fec_decode_batch-style launch; on that path a
 * device-side pattern_of is first copied to the host, which SYNCHRONISES the
 * stream.  While the stream is being captured into a graph the call returns
 * FEC_EINVAL. */
int fec_decode_batch_mixed(const fec_t* code,
                           const gf* src, size_t src_block_stride, size_t src_stripe_stride,
                           gf* dst, size_t dst_block_stride, size_t dst_stripe_stride,
                           const unsigned* patterns, size_t npatterns,
                           const unsigned* pattern_of,
                           size_t sz, size_t nstripes, void* stream, unsigned flags);

/* Host only, no GPU: the k x k matrix fec_decode_batch_mixed applies for one
 * pattern (row i yields primary i from the k slots), row-major into rows[k*k].
 * FEC_OK / FEC_EINVAL / FEC_ESINGULAR. */
int fec_mixed_decode_rows(const fec_t* code, const unsigned* pattern, gf* rows);

/* Batched parity verification (scrubbing): are the blocks a store holds still
 * consistent with each other?  Nothing is written but a few bits per stripe.
 *
 * Every stripe holds nb = num_block_nums blocks: slot j of stripe s at
 * src + s*src_stripe_stride + j*src_block_stride holds block block_nums[j].
 * The numbers are distinct, all < n, in any order, and k + 1 <= nb <= n.  The
 * first k slots are the basis, the other c = nb - k slots the checks.  Check i
 * (slot k + i) is consistent when, over all sz bytes, it equals row i of
 * P = E[checks] . inverse(E[basis]) applied to the basis blocks (E: the code's
 * enc_matrix).  With the basis 0..k-1 in order P is the encode rows of the
 * check blocks: the common "primaries against parity" scrub.
 *
 * Result: W = ceil(c / 32) words per stripe.  Bit i % 32 of
 * mismatch[s*W + i/32] is set iff check i of stripe s differs in at least one
 * byte; every other bit is 0.  The library clears the nstripes x W words
 * itself, in stream order, before its kernels run; they never write to src.
 *
 * Reading the mask: the code is MDS, so P has no zero entry.  A corrupt check
 * block sets exactly its own bit; ONE corrupt basis block sets all c bits of
 * its stripe; fec_locate_batch below names that block.
 *
 * src: device memory on one device, or page-locked host memory read in place;
 * pageable host memory returns FEC_EINVAL (this call does not stage).  A
 * block-major layout is walked stripe by stripe.  mismatch in device memory is
 * used in place (on the blocks' device, else FEC_EINVAL) and FEC_FLAG_ASYNC is
 * honoured.  mismatch in host memory, pageable or page-locked: the kernels use
 * device-scope atomics, which must not be aimed at host memory over PCIe, so
 * the library gathers the words in device memory it owns and copies them back;
 * the call is then synchronous whatever the flags.  FEC_FLAG_LIBRARY_STREAM as
 * elsewhere; FEC_FLAG_ROW_PADDING is accepted and ignored.  While the stream is
 * being captured into a graph the call returns FEC_EINVAL.
 *
 * Checked before any GPU work, in this order, each FEC_EINVAL with a message:
 * invalid fec_t; NULL src, block_nums or mismatch; nb <= k ("nothing to
 * check"); nb > n; a block number >= n; a duplicate.  Then FEC_ENODEV when no
 * GPU is visible.  nstripes == 0 returns FEC_OK; sz == 0 returns FEC_OK with the
 * words cleared.
 *
 * k <= 4 runs on matverify_reg<k, r> (at most 8 checks per launch): the check
 * rows are recomputed in registers and compared, so the call reads every block
 * once and, on clean data, writes nothing.  4 < k <= 32 with blocks of at
 * least 2048 bytes in device memory runs on matverify_bsr<rt>, <rt,lds> or
 * <rt,lds,tbl> (at most 40 checks per launch) once the call has
 * ZFEC_HIP_VERIFY_FUSED_MIN units of 2 KiB (ceil(sz / 2048) x nstripes): the
 * bit-sliced encode walk with the check rows kept as bit-planes in registers
 * and compared there, so these calls too read every block once, write nothing
 * on clean data and need no scratch (calls on different streams do not wait
 * for each other).  Everything else -- smaller calls, shorter blocks, k > 32,
 * page-locked host blocks -- computes the expected rows into library scratch
 * (at most 64 MiB per device, batches cut to fit) with the encode kernels and
 * compares them with rows_differ. */
int fec_verify_batch(const fec_t* code,
                     const gf* src, size_t src_block_stride, size_t src_stripe_stride,
                     const unsigned* block_nums, size_t num_block_nums,
                     size_t sz, size_t nstripes,
                     unsigned* mismatch, void* stream, unsigned flags);

/* Host only, no GPU: the c x k matrix P fec_verify_batch applies for
 * block_nums (row i yields the block of slot k + i from the k basis slots),
 * row-major into rows[c*k].  FEC_OK / FEC_EINVAL / FEC_ESINGULAR. */
int fec_verify_rows(const fec_t* code, const unsigned* block_nums, size_t num_block_nums, gf* rows);

/* Batched single-block error location: which block of an inconsistent stripe
 * is the corrupt one?  The step between fec_verify_batch and fec_repair_batch:
 * scrub, locate and repair are three calls with no host round trip.
 *
 * Arguments as in fec_verify_batch: nb = k + c blocks per stripe, slot j holds
 * block block_nums[j], the first k slots the basis, the other c the checks, and
 * P = E[checks] . inverse(E[basis]) (fec_verify_rows; no zero entry).  At every
 * byte position the syndromes are
 *     s_i = stored check i ^ sum_j P[i][j] . basis_j,   i = 0..c-1,
 * the words fec_verify_batch reduces to one bit each.  For c >= 2 let
 * Q[i][j] = P[i][j] / P[0][j], i = 1..c-1 (fec_locate_rows).  Per stripe, over
 * all sz bytes:
 *   mismatch bit i is set iff s_i != 0 somewhere (exactly the verify bits);
 *   excluded bit j (j < k) is set iff s_i != Q[i][j] . s_0 somewhere, for some
 *     i >= 1: the hypothesis "only basis slot j is corrupt" is refuted.
 * culprit[s], one unsigned per stripe, is
 *   1. FEC_LOCATE_CLEAN when no mismatch bit is set;
 *   2. otherwise FEC_LOCATE_UNKNOWN when c == 1 (any of the k + 1 blocks could
 *      be the bad one);
 *   3. otherwise k + i0 when exactly one mismatch bit i0 is set: a check block;
 *   4. otherwise j when exactly one basis slot j is not excluded;
 *   5. otherwise FEC_LOCATE_MANY.
 * A value below nb is a SLOT index into block_nums, not a block number.
 *
 * What this guarantees (the held blocks form an MDS code, so any c columns of
 * [P | I] are independent).  With c >= 2 a stripe with exactly one corrupt
 * block gets that block's slot, whatever the bytes.  Two corrupt blocks at
 * different byte positions always give MANY; two to c - 1 corrupt blocks at the
 * same byte position give MANY (this needs c >= 3).  From c blocks corrupt at
 * one position on the verdict can be wrong, as with any decoder past its
 * distance: with c = 2 that is already two blocks.  At most one basis slot can
 * survive in rule 4.
 *
 * src as in fec_verify_batch: device memory on one device, or page-locked host
 * memory read in place; pageable host memory returns FEC_EINVAL.  A block-major
 * layout is walked stripe by stripe.  culprit in device memory is used in place
 * (on the blocks' device, else FEC_EINVAL) and FEC_FLAG_ASYNC is honoured;
 * culprit in host memory is gathered in device memory the library owns and
 * copied back, and the call is then synchronous whatever the flags.
 * FEC_FLAG_LIBRARY_STREAM as elsewhere; FEC_FLAG_ROW_PADDING is accepted and
 * ignored.  While the stream is being captured into a graph the call returns
 * FEC_EINVAL.  src is never written, and nothing outside the nstripes verdict
 * words is written in caller memory: the per-stripe bits are kept in device
 * memory the library owns (the kernels' device-scope atomics aim only there).
 *
 * Checked before any GPU work, in this order, each FEC_EINVAL with a message:
 * invalid fec_t; NULL src, block_nums or culprit; nb <= k ("nothing to
 * check"); nb > n; a block number >= n; a duplicate.  Then FEC_ENODEV when no
 * GPU is visible.  nstripes == 0 returns FEC_OK; sz == 0 returns FEC_OK with
 * every verdict FEC_LOCATE_CLEAN.
 *
 * k <= 4 with 2 <= c <= 8 runs on matlocate_reg<k, c>, one launch:
 * matverify_reg's walk with the syndromes kept in registers, the k hypotheses
 * tested only in waves that saw a nonzero syndrome, so clean data costs what
 * fec_verify_batch costs.  c == 1 runs the verify kernels.  Other codes compute
 * the expected rows into library scratch as fec_verify_batch does and compare
 * with rows_locate.  locate_finish then writes the verdicts;
 * fec_last_kernel_name() names the kernel that read the blocks. */
#define FEC_LOCATE_CLEAN   0xFFFFFFFFu
#define FEC_LOCATE_MANY    0xFFFFFFFEu
#define FEC_LOCATE_UNKNOWN 0xFFFFFFFDu
int fec_locate_batch(const fec_t* code,
                     const gf* src, size_t src_block_stride, size_t src_stripe_stride,
                     const unsigned* block_nums, size_t num_block_nums,
                     size_t sz, size_t nstripes,
                     unsigned* culprit, void* stream, unsigned flags);

/* Host only, no GPU: the (c-1) x k matrix Q fec_locate_batch tests with,
 * row-major into rows[(c-1)*k]; c == 1 writes nothing.
 * FEC_OK / FEC_EINVAL / FEC_ESINGULAR. */
int fec_locate_rows(const fec_t* code, const unsigned* block_nums, size_t num_block_nums, gf* rows);

/* Ragged scrub: fec_verify_batch and fec_locate_batch over stripes that each
 * have their own size (the arena of fec_encode_batch_ragged), in one launch.
 *
 * Stripe s holds nb = num_block_nums blocks of sizes[s] bytes; slot j starts at
 * src + src_offsets[s] + j*B, with B = src_block_stride when that is nonzero and
 * B = sizes[s] otherwise: the packed object [slot 0 | ... | slot nb-1].  A
 * nonzero stride describes block-major arenas.  Offsets are arbitrary bytes.
 * block_nums means exactly what it means to fec_verify_batch: nb distinct
 * numbers below n in any order, the first k slots the basis, the other
 * c = nb - k the checks.
 *
 * The results are those of the uniform calls made once per stripe with
 * nstripes = 1 and sz = sizes[s]: fec_verify_batch_ragged returns W =
 * ceil(c/32) words per stripe in mismatch[s*W ..], bit i set iff check i
 * differs somewhere and every other bit 0; fec_locate_batch_ragged one verdict
 * word per stripe by rules 1-5 of fec_locate_batch.  A zero-size stripe is
 * neither read nor judged dirty: its words are 0, its verdict
 * FEC_LOCATE_CLEAN.  The library clears the result words itself, in stream
 * order.  src is never written, and nothing in caller memory outside the
 * result words is.
 *
 * sizes and src_offsets are two arrays of nstripes 8-byte words (8-byte
 * aligned), both in host memory or both in device memory on the blocks'
 * device; a mix returns FEC_EINVAL.  Host arrays are copied when the call is
 * made and may be reused when it returns; device arrays are read where they
 * are, in stream order, and nothing synchronises the stream.
 *
 * src_bytes is the extent of the arena.  A stripe with sizes[s] > 0 FITS when
 * offset + (nb - 1)*B + sizes[s] <= src_bytes, evaluated without wrapping.
 * With host arrays a stripe that does not fit is FEC_EINVAL, the message naming
 * the stripe.  With device arrays such a stripe is not read and the result
 * MARKS it: fec_verify_batch_ragged sets all c check bits of the stripe (a
 * scrub must not vouch for what it did not read), fec_locate_batch_ragged
 * writes FEC_LOCATE_UNFIT; no error is returned.  This departs on purpose
 * from the "left untouched" rule of the writing ragged calls: there untouched
 * output is the safe outcome, here a cleared word would read as "clean".
 *
 * src is device memory on one device, or page-locked host memory read in
 * place; pageable host memory returns FEC_EINVAL.  mismatch / culprit in device
 * memory is used in place and FEC_FLAG_ASYNC is honoured; in host memory it is
 * gathered in device words the library owns and copied back, and the call is
 * synchronous.  Every atomic aims at device memory the library owns or at the
 * caller's device-side mismatch words, never at host memory.
 * FEC_FLAG_LIBRARY_STREAM as elsewhere; FEC_FLAG_ROW_PADDING is accepted and
 * ignored.  While the stream is being captured into a graph the call returns
 * FEC_EINVAL.
 *
 * Checked before any GPU work, in this order, each FEC_EINVAL with a message
 * naming the call: an invalid fec_t; a NULL src, sizes, src_offsets,
 * block_nums or mismatch / culprit; nb <= k ("nothing to check"); nb > n; a
 * block number >= n; a duplicate; nstripes >= 2^32; descriptor arrays of mixed
 * memory kinds; with host arrays a stripe that does not fit.  Then FEC_ENODEV
 * when no GPU is visible.  nstripes == 0 returns FEC_OK.
 *
 * k <= 4 runs matverify_ragged<k,r> (one launch per 8 checks) or, with
 * 2 <= c <= 8, matlocate_ragged<k,c>: matapply_ragged's walk around the unit
 * of matverify_reg / matlocate_reg, the bits accumulated per (wave, stripe) and
 * OR-ed out once where nonzero, so clean data performs no store and no atomic;
 * locate_finish forms the verdicts after the launch.  c == 1 locates with
 * matverify_ragged (FEC_LOCATE_UNKNOWN for a dirty stripe).  With device
 * arrays ragged_scan and a one-lane-per-stripe marking kernel run in the same
 * stream.  Other shapes (k > 4; a location with c > 8) are cut into runs of
 * consecutive stripes of one size whose offset advances by a constant, each
 * run one fec_verify_batch / fec_locate_batch-style launch (at worst one per
 * stripe); on that path device-side arrays are first copied to the host, which
 * SYNCHRONISES the stream.  fec_last_kernel_name() names the kernel that read
 * the blocks last. */
#define FEC_LOCATE_UNFIT   0xFFFFFFFBu
int fec_verify_batch_ragged(const fec_t* code,
                            const gf* src, size_t src_bytes, size_t src_block_stride,
                            const unsigned long long* src_offsets,
                            const unsigned long long* sizes,
                            const unsigned* block_nums, size_t num_block_nums,
                            size_t nstripes,
                            unsigned* mismatch, void* stream, unsigned flags);
int fec_locate_batch_ragged(const fec_t* code,
                            const gf* src, size_t src_bytes, size_t src_block_stride,
                            const unsigned long long* src_offsets,
                            const unsigned long long* sizes,
                            const unsigned* block_nums, size_t num_block_nums,
                            size_t nstripes,
                            unsigned* culprit, void* stream, unsigned flags);

/* Batched in-place correction: scrub, locate and heal in ONE call.  The
 * arguments are exactly those of fec_locate_batch, except that `blocks` is
 * writable.  Over all sz bytes of each stripe:
 *
 *   1. culprit[s] receives exactly the verdict fec_locate_batch would give for
 *      the blocks as they were on entry (rules 1-5 above).
 *   2. For a stripe whose verdict is a slot h < nb, the sz bytes of slot h are
 *      rewritten from k other slots of that stripe: the sources S_h are slots
 *      0..k-1 for h >= k; for h < k they are 0..k-1 with slot h replaced by
 *      slot k (check 0).  The row applied is row h of the nb x k matrix
 *      fec_correct_rows returns: P[h-k] for h >= k; for h < k,
 *      R[l] = P[0][l] / P[0][h] for l != h and R[h] = 1 / P[0][h] (check 0's
 *      equation solved for slot h).  Equivalently, row h is
 *      fec_repair_rows(present = block_nums[S_h], targets = {block_nums[h]}).
 *   3. Nothing else in caller memory is written: no byte of a CLEAN, MANY or
 *      UNKNOWN stripe; in a corrected stripe no slot but h; no byte past sz of
 *      slot h (row slack, other stripes); nothing around the nstripes verdict
 *      words.  A stripe that is not corrected is not read again after the scrub.
 *
 * Every stripe that gets a slot verdict is a codeword afterwards.  Let e be
 * what the rewrite adds to slot h at some byte position, and s_i the
 * syndromes on entry.  A verdict h means s_i = P[i][h] . d at every byte for
 * one d per byte (P[i][h] read as the unit column for a check slot: rule 3
 * or rule 4), and the row above yields e = d.  So
 *     s_i' = s_i ^ P[i][h] . e = 0   for every i,
 * and fec_verify_batch on the stripe returns no bit, whatever the corruption
 * was.  The correction guarantees are those of locate: with c >= 2, exactly one
 * corrupt block is restored bit for bit; from c blocks corrupt at one byte
 * position on, a MIScorrection is possible -- the stripe becomes a codeword, but
 * not the one that was stored -- and with c = 2 that is already two blocks, so a
 * caller who wants double errors refused passes c >= 3; with c = 1 no verdict
 * is a slot and nothing is ever rewritten.
 *
 * Memory, streams, capture and validation follow fec_locate_batch: blocks are
 * device memory on one device, or page-locked host memory read AND WRITTEN in
 * place (plain vector stores only; the atomics stay aimed at device words the
 * library owns); pageable memory returns FEC_EINVAL; a block-major layout is
 * walked stripe by stripe; culprit in device memory is used in place and
 * FEC_FLAG_ASYNC is honoured; culprit in host memory goes through device words
 * the library owns (the correction reads those) and the call is then
 * synchronous; under graph capture the call returns FEC_EINVAL.  The checks
 * and their order are fec_locate_batch's, the messages naming
 * fec_correct_batch.  nstripes == 0 returns FEC_OK; sz == 0 returns FEC_OK with
 * every verdict FEC_LOCATE_CLEAN and nothing written.  Slots and stripes must
 * not overlap in memory.
 *
 * The location runs exactly as in fec_locate_batch.  One correction follows it
 * in the same stream over the verdict words in device memory (the host never
 * sees them): matcorrect_reg<k> for k <= 4 -- whatever kernel located --
 * and rows_correct past that.  A wave reads its stripe's verdict by a scalar
 * load before anything else and skips the stripe unless it names a slot.
 * fec_last_kernel_name() names the correction kernel. */
int fec_correct_batch(const fec_t* code,
                      gf* blocks, size_t block_stride, size_t stripe_stride,
                      const unsigned* block_nums, size_t num_block_nums,
                      size_t sz, size_t nstripes,
                      unsigned* culprit, void* stream, unsigned flags);

/* Host only, no GPU: the nb x k matrix fec_correct_batch applies (row h
 * rebuilds slot h from its sources S_h, in slot order), row-major into
 * rows[nb*k].  FEC_OK / FEC_EINVAL / FEC_ESINGULAR. */
int fec_correct_rows(const fec_t* code, const unsigned* block_nums, size_t num_block_nums, gf* rows);

/* Two corrupt blocks per stripe: fec_locate2_batch names them, and
 * fec_correct2_batch heals them in place.  The arguments are those of
 * fec_locate_batch / fec_correct_batch, except that culprit holds TWO words
 * per stripe in planar layout: culprit[s] is the first word of stripe s and
 * culprit[nstripes + s] the second, 2 * nstripes words in all.
 *
 * Let p_h be column h of the c x nb matrix [P | I]: P's column for a basis
 * slot, a unit column for a check slot, so that the syndrome vector at a byte
 * is s = sum_h e_h . p_h over the slots' error bytes e_h.
 *   Rules 1-4 of fec_locate_batch are unchanged: they give CLEAN, UNKNOWN or a
 *     single slot h as the first word; the second word is FEC_LOCATE_NONE.
 *   Rule 5 applies where fec_locate_batch says MANY, when c >= 4 and nb <= 32.
 *     The pair hypothesis (a, b), a < b < nb, "only slots a and b are corrupt"
 *     is refuted iff at some byte s is not in span(p_a, p_b).  If exactly one
 *     pair is not refuted the verdict is (a, b); otherwise it is
 *     (FEC_LOCATE_MANY, FEC_LOCATE_NONE).
 *   With c < 4 or nb > 32 the pair pass does not run: the first word is
 *     exactly fec_locate_batch's verdict, the second is FEC_LOCATE_NONE, and no
 *     error is returned.
 * Where a pair needs an index it is p = a*nb - a(a+1)/2 + (b - a - 1)
 * (lexicographic order).
 *
 * What this guarantees.  Any c columns of [P | I] are independent (the held
 * blocks form an MDS code); four columns need c >= 4.
 *   - A stripe with exactly two corrupt blocks a, b gets (a, b), whether they
 *     differ at the same bytes or at different ones: every s lies in
 *     span(p_a, p_b), so (a, b) is never refuted.  Another pair (a', b')
 *     survives only if every s lies in span(p_a', p_b') too; the two spans
 *     meet in 0 when the pairs are disjoint and in one column's line when
 *     they share a slot (else three or four columns were dependent), so all
 *     the errors would sit in at most one block -- which rules 3 and 4 catch.
 *   - At most one pair survives under rule 5, by the same argument: two
 *     surviving pairs put every s on one column's line, a single-block
 *     stripe, and those never reach rule 5.
 *   - A stripe with one corrupt block gets that slot by rules 3-4.
 *   - Three to c - 2 blocks corrupt at one byte give MANY (this needs c >= 5):
 *     s is a combination of t <= c - 2 columns with nonzero weights, and were
 *     it in some span(p_a, p_b), at most t + 2 <= c columns were dependent.
 *   - From c - 1 blocks corrupt at one byte on, a wrong pair is possible, as
 *     with any decoder past its distance.  With c = 4 that is already three
 *     blocks: pass c >= 5 to have triple errors refused.
 *
 * fec_correct2_batch: verdicts are exactly fec_locate2_batch's for the blocks
 * as they were on entry.  A single-slot verdict is healed exactly as
 * fec_correct_batch heals it.  For a pair verdict (a, b) the sz bytes of slots
 * a and b are rewritten: the sources S_ab are the k lowest-numbered slots not
 * in {a, b}, ascending, and the rows are fec_repair_rows(present =
 * block_nums[S_ab], targets = {block_nums[a], block_nums[b]})
 * (fec_correct2_rows).  Nothing else in caller memory is written (the list of
 * fec_correct_batch's rule 3).  Every stripe that gets a slot or pair verdict
 * passes fec_verify_batch afterwards, whatever the corruption was: a surviving
 * pair means some codeword differs from the stored blocks only in a and b, and
 * rebuilding a and b from any k other blocks yields it.
 *
 * Memory, streams, flags, capture (FEC_EINVAL under capture) and the order of
 * validation are fec_locate_batch's, the messages naming the new calls.
 * culprit is device memory used in place (FEC_FLAG_ASYNC honoured) or host
 * memory gathered in device words the library owns and copied back.  sz == 0
 * gives (CLEAN, NONE) everywhere.  Page-locked host blocks are read, and by
 * fec_correct2_batch written, in place with plain vector stores; every atomic
 * aims at device memory the library owns.
 *
 * The location path of fec_locate_batch runs unchanged, so clean data pays
 * what it pays there plus the second plane's stores and the launches below
 * over an empty list.  locate2_finish writes both planes and appends every
 * MANY stripe to a dirty list in device memory; (fec_correct2_batch: the
 * single-slot correction of fec_correct_batch runs here;) pairs_locate walks
 * the list, forms the c syndromes of each unit and ORs refuted pair bits into
 * the entry's words; pairs_finish names the one surviving pair; pairs_correct
 * rewrites it.  fec_last_kernel_name() is pairs_locate after
 * fec_locate2_batch and pairs_correct after fec_correct2_batch where the pair
 * pass runs (sz != 0, c >= 4, nb <= 32), else what the single-block call
 * reports. */
#define FEC_LOCATE_NONE    0xFFFFFFFCu
int fec_locate2_batch(const fec_t* code,
                      const gf* src, size_t src_block_stride, size_t src_stripe_stride,
                      const unsigned* block_nums, size_t num_block_nums,
                      size_t sz, size_t nstripes,
                      unsigned* culprit, void* stream, unsigned flags);
int fec_correct2_batch(const fec_t* code,
                       gf* blocks, size_t block_stride, size_t stripe_stride,
                       const unsigned* block_nums, size_t num_block_nums,
                       size_t sz, size_t nstripes,
                       unsigned* culprit, void* stream, unsigned flags);

/* Host only, no GPU: a (c-2) x c matrix N of rank c - 2 with N . p_a =
 * N . p_b = 0, row-major into rows[(c-2)*c]: s lies in span(p_a, p_b) iff
 * N . s = 0.  The pivot form is written: two rows r0, r1 on which [p_a p_b]
 * has a nonzero minor, and for every other row i the row e_i + alpha . e_r0 +
 * beta . e_r1.  FEC_EINVAL for a >= b, b >= nb or c < 4, after
 * fec_locate_rows' checks.  FEC_OK / FEC_EINVAL / FEC_ESINGULAR. */
int fec_locate2_rows(const fec_t* code, const unsigned* block_nums, size_t num_block_nums, unsigned a, unsigned b,
                     gf* rows);

/* Host only, no GPU: sources[k], the k lowest-numbered slots not in {a, b},
 * ascending, and rows[2*k], row-major, the coefficients that yield slot a
 * (row 0) and slot b (row 1) from them.  FEC_EINVAL for a >= b, b >= nb or
 * c < 2.  FEC_OK / FEC_EINVAL / FEC_ESINGULAR. */
int fec_correct2_rows(const fec_t* code, const unsigned* block_nums, size_t num_block_nums, unsigned a, unsigned b,
                      unsigned* sources, gf* rows);

/* Batched repair: rebuild any lost blocks of every stripe, primaries and parity
 * alike, from the k blocks the stripe still holds, in one call (the step after
 * fec_verify_batch in a store's scrub-and-repair cycle).
 *
 * present: npatterns x k block numbers (host memory); targets: npatterns x
 * ntargets block numbers or FEC_REPAIR_NONE (host memory).  Stripe s uses
 * pattern p = pattern_of[s]: slot j of the stripe, at src + s*src_stripe_stride
 * + j*src_block_stride, holds block present[p*k+j] (k distinct numbers < n, in
 * ANY slot order, as in fec_decode_batch_mixed), and output row i of the stripe,
 * at dst + s*dst_stripe_stride + i*dst_block_stride, receives block
 * targets[p*ntargets+i] of that stripe: exactly the bytes fec_decode followed
 * by fec_encode of that block number would produce (the primary itself for a
 * number below k).  The matrix applied is row i = E[target i] . inverse(E[present])
 * (E: the code's enc_matrix).  A target may be any number < n: one that is also
 * present gives a unit row, so its output is a copy; duplicates within a
 * pattern are allowed, every output row being independent.
 *
 * A FEC_REPAIR_NONE target marks a row its pattern does not use: the row is NOT
 * written, none of its sz bytes and nothing past them.  So one call serves
 * stripes that lost different numbers of blocks: ntargets is the batch's
 * maximum, shorter lists are filled with FEC_REPAIR_NONE, and a pattern whose
 * targets are all FEC_REPAIR_NONE leaves its stripes untouched.
 * 1 <= ntargets <= 32, npatterns <= 65536.
 *
 * pattern_of: nstripes pattern ids (unsigned, 4 bytes each) in host OR device
 * memory.  Ids in DEVICE memory cannot be checked by the host: a stripe whose id
 * is >= npatterns is left unwritten (no table is read for it), and no error is
 * reported.  pattern_of == NULL requires npatterns == 1: every stripe uses
 * pattern 0, and the call is one shared-matrix application of the pattern's
 * rows (FEC_REPAIR_NONE rows dropped from the launch) by whatever kernel
 * fec_encode_batch would pick for that shape, graph capture included.
 *
 * src and dst are device memory on one device, or page-locked host memory;
 * pageable host memory returns FEC_EINVAL (this call does not stage).  dst must
 * not overlap src: the result is then unspecified.  Strides as in
 * fec_decode_batch_mixed.  FEC_FLAG_ASYNC and FEC_FLAG_LIBRARY_STREAM as there;
 * FEC_FLAG_ROW_PADDING is accepted and ignored.  With pattern_of non-NULL the
 * call returns FEC_EINVAL while the stream is being captured into a graph (the
 * pattern tables are uploaded, through staging the library owns, when the call
 * is made; present, targets and pattern_of may be reused as soon as it returns).
 *
 * Checked before any GPU work, in this order, each FEC_EINVAL with a message
 * naming the pattern or stripe: invalid fec_t; NULL src, dst, present or
 * targets; ntargets == 0 or > 32; npatterns == 0 with stripes to repair, or
 * more than 65536 patterns; pattern_of == NULL with npatterns != 1; a present
 * number >= n; a duplicate among a pattern's present numbers; a target that is
 * neither < n nor FEC_REPAIR_NONE; an id >= npatterns in a HOST-side
 * pattern_of.  Then FEC_ENODEV when no GPU is visible.  nstripes == 0 or
 * sz == 0 returns FEC_OK.
 *
 * k <= 4 runs on matrepair_mixed<k, r>, at most 8 rows per launch (11 targets
 * are launches of 8 and 3 rows over one upload of the tables; a group of rows
 * that no pattern uses is skipped).  4 < k <= 32 with sz >= 2048 and the blocks
 * in device memory runs as ONE launch of matapply_bsr<RT,mix> (ntargets <= 10)
 * or matapply_bsr<RT,lds,mix>, over one record per pattern (its rows' routine
 * addresses and a live-row mask) uploaded through the same staging; a
 * device-side pattern_of is read where it is and nothing synchronises the
 * stream; a call whose targets are all FEC_REPAIR_NONE launches nothing.  The
 * remaining shapes -- k > 32, sz < 2048, page-locked host blocks, more than 32
 * MiB of records, no routine table on the device, ZFEC_HIP_MIXED_FUSED=0 -- are
 * cut into runs of consecutive stripes with one id, each run one shared-matrix
 * launch of that pattern's used rows; on that path a device-side pattern_of is
 * first copied to the host, which SYNCHRONISES the stream. */
#define FEC_REPAIR_NONE 0xFFFFFFFFu /* a target slot this pattern does not use */
int fec_repair_batch(const fec_t* code,
                     const gf* src, size_t src_block_stride, size_t src_stripe_stride,
                     gf* dst, size_t dst_block_stride, size_t dst_stripe_stride,
                     const unsigned* present, const unsigned* targets,
                     size_t ntargets, size_t npatterns,
                     const unsigned* pattern_of,
                     size_t sz, size_t nstripes, void* stream, unsigned flags);

/* Host only, no GPU: the ntargets x k matrix fec_repair_batch applies for one
 * pattern (row i yields block targets[i] from the k slots; a FEC_REPAIR_NONE
 * row is all zeros), row-major into rows[ntargets*k].  The same checks on the
 * one pattern.  FEC_OK / FEC_EINVAL / FEC_ESINGULAR. */
int fec_repair_rows(const fec_t* code, const unsigned* present, const unsigned* targets, size_t ntargets,
                    gf* rows);

/* Pattern plans: a store has a small, stable set of erasure patterns, so the
 * per-pattern work of fec_repair_batch -- one k x k inversion on the host, the
 * tables or routine-address records, their upload -- is done once and reused.
 *
 * fec_repair_plan_new takes the pattern arguments of fec_repair_batch (present,
 * targets, ntargets, npatterns; a decode plan is targets = 0..k-1 for every
 * pattern, so it needs k <= 32) and checks them in the same order with the same
 * messages: invalid fec_t; NULL present, targets or plan; ntargets == 0 or > 32;
 * npatterns == 0 or more than 65536 patterns; a present number >= n; a
 * duplicate among a pattern's present numbers; a target that is neither < n nor
 * FEC_REPAIR_NONE.  Then FEC_ENODEV when no GPU is visible, FEC_EINVAL for a
 * device that does not exist (-1: the current device).  The plan owns the
 * host-side rows and masks and, in device memory of its own on that device, the
 * records: matrepair_mixed's for k <= 4, matapply_bsr<..,mix>'s for 4 < k <= 32
 * (none for k > 32, or where the device has no routine table: such a plan's
 * calls take the run path).  It returns with the upload complete.  Plans are
 * immutable: any thread may use one, concurrently, on any streams.
 * fec_repair_plan_free(NULL) is harmless; a plan must outlive the calls (and
 * graphs) that use it.
 *
 * fec_repair_batch_planned is fec_repair_batch with the plan in place of the
 * pattern arguments: the same buffer rules, flags, strides and output, byte for
 * byte.  pattern_of must not be NULL; blocks or device-side ids on another
 * device than the plan's return FEC_EINVAL.  k <= 4 launches matrepair_mixed
 * over the plan's records (row groups of 8), 4 < k <= 32 with sz >= 2048 and
 * device blocks the mix form of matapply_bsr; everything else takes the run
 * path from the plan's host rows.  With pattern_of in DEVICE memory those two
 * launches touch nothing the library owns and reuses, so the call MAY BE
 * CAPTURED INTO A GRAPH; with host-side ids (staged per call) it returns
 * FEC_EINVAL under capture as fec_repair_batch does. */
typedef struct fec_repair_plan fec_repair_plan_t;
int fec_repair_plan_new(const fec_t* code, const unsigned* present, const unsigned* targets,
                        size_t ntargets, size_t npatterns, int device, fec_repair_plan_t** plan);
void fec_repair_plan_free(fec_repair_plan_t* plan);
int fec_repair_batch_planned(const fec_repair_plan_t* plan,
                             const gf* src, size_t src_block_stride, size_t src_stripe_stride,
                             gf* dst, size_t dst_block_stride, size_t dst_stripe_stride,
                             const unsigned* pattern_of, size_t sz, size_t nstripes,
                             void* stream, unsigned flags);

/* Batched parity update: bring the stored blocks of every stripe up to date
 * after some of its primaries changed, from the changed blocks alone (the
 * small-write path of a store; fec_encode_batch needs all k primaries).  The
 * code is linear, so for every stored block b and changed primary j
 *     block_b(new stripe) = block_b(old stripe) ^ E[b][j] . (old_j ^ new_j)
 * with E the code's enc_matrix.  A parity node that holds a few parity blocks
 * and no primary calls this with the delta it received; a node that holds whole
 * wide stripes reads 1 + r blocks and writes r instead of reading k.
 *
 * rows: row i of stripe s, at rows + s*row_stripe_stride + i*row_block_stride,
 * holds block block_nums[i] of that stripe: num_block_nums distinct numbers
 * < n (host memory), in any order, 1 <= num_block_nums <= n.  Primaries are
 * allowed (their row of E is a unit row).  The rows are updated IN PLACE.
 *
 * changed: nstripes x nchanged numbers (unsigned, 4 bytes each) in host OR
 * device memory (on the blocks' device), 1 <= nchanged <= 4: word
 * [s*nchanged + c] is the number of the primary that input slot c of stripe s
 * carries, or FEC_UPDATE_NONE.  Input slot c of stripe s is at
 * base + s*in_stripe_stride + c*in_block_stride, in newb and in oldb alike.
 * With oldb == NULL newb holds the deltas d = old ^ new themselves; otherwise
 * the kernel forms d from the two.
 *
 * Every slot that is not FEC_UPDATE_NONE contributes E[block_nums[i]][j] . d to
 * row i.  Slots are independent and their contributions XOR together, so the
 * same number in two slots is allowed (the two add).  Afterwards each stored
 * row holds exactly the bytes fec_encode of that block number gives on the
 * stripe with the new primaries; a stored primary row that names a changed
 * block holds the new block.  A FEC_UPDATE_NONE slot is not read.  A row whose
 * coefficients for the stripe's live slots are all zero (this can only be a
 * primary row) is neither read nor written, and a stripe whose slots are all
 * FEC_UPDATE_NONE is untouched.  Nothing outside the sz bytes of a row is
 * written.  The inputs must not overlap the rows: the result is then
 * unspecified.
 *
 * Numbers in HOST memory are checked: one that is neither < k nor
 * FEC_UPDATE_NONE is FEC_EINVAL, naming the stripe and the slot.  Numbers in
 * DEVICE memory cannot be seen by the host: such a slot is treated as
 * FEC_UPDATE_NONE and no error is reported (the rule a device-side pattern_of
 * follows in fec_repair_batch).
 *
 * oldb, newb and rows are device memory on one device, or page-locked host
 * memory; pageable host memory returns FEC_EINVAL (this call does not stage).
 * FEC_FLAG_ASYNC and FEC_FLAG_LIBRARY_STREAM as in fec_repair_batch;
 * FEC_FLAG_ROW_PADDING is accepted and ignored.  The call returns FEC_EINVAL
 * while the stream is being captured into a graph (its coefficient records are
 * uploaded, through staging the library owns, when the call is made;
 * block_nums and a host-side changed may be reused as soon as it returns).
 *
 * Checked before any GPU work, in this order, each FEC_EINVAL with a message:
 * invalid fec_t; NULL newb, rows, block_nums or changed; num_block_nums == 0 or
 * > n; a block number >= n; a duplicate block number; nchanged == 0 or > 4;
 * nstripes >= 2^32; a bad number in a HOST-side changed.  Then FEC_ENODEV when
 * no GPU is visible.  nstripes == 0 or sz == 0 returns FEC_OK.
 *
 * Every code runs on matupdate_reg<nchanged, r>: one column of E per changed
 * block is involved, so the kernel does not depend on k.  A launch takes at
 * most 8 rows; more run as row groups of 8 over one upload, EACH RE-READING THE
 * INPUTS (the 40 parity rows of K=20/M=60 are 5 launches).  Nothing
 * synchronises the stream. */
#define FEC_UPDATE_NONE 0xFFFFFFFFu /* a slot of `changed` this stripe does not use */
int fec_update_batch(const fec_t* code,
                     const gf* oldb, const gf* newb,
                     size_t in_block_stride, size_t in_stripe_stride,
                     gf* rows, size_t row_block_stride, size_t row_stripe_stride,
                     const unsigned* block_nums, size_t num_block_nums,
                     const unsigned* changed, size_t nchanged,
                     size_t sz, size_t nstripes, void* stream, unsigned flags);

/* Host only, no GPU: coefs[i] = E[block_nums[i]][changed_block], the
 * coefficient fec_update_batch multiplies the delta of primary changed_block
 * by for stored row i.  The same checks on code, block_nums (and coefs) and
 * the numbers; changed_block >= k is FEC_EINVAL.  FEC_OK / FEC_EINVAL. */
int fec_update_rows(const fec_t* code, const unsigned* block_nums, size_t num_block_nums,
                    unsigned changed_block, gf* coefs);

/* Ragged repair: fec_repair_batch over stripes that each have their own size,
 * in one launch.  The arena arguments are those of fec_encode_batch_ragged,
 * the pattern arguments those of fec_repair_batch.
 *
 * Slot j of stripe s starts at src + src_offsets[s] + j*B, with B =
 * src_block_stride, or sizes[s] when the stride is 0; output row i starts at
 * dst + dst_offsets[s] + i*B', B' formed the same way from dst_block_stride.
 * Offsets are arbitrary bytes.  A zero-size stripe is neither read nor
 * written.  Stripe s uses pattern p = pattern_of[s]: slot j holds block
 * present[p*k + j], in any slot order, and row i receives block
 * targets[p*ntargets + i].  A FEC_REPAIR_NONE row is not written: none of its
 * bytes and nothing past them.  pattern_of == NULL requires npatterns == 1,
 * and every stripe then uses pattern 0.  The bytes are those of
 * fec_repair_batch called once per stripe with nstripes = 1 and sz = sizes[s].
 * A decode with a pattern per stripe is this call with targets 0..k-1.
 *
 * sizes, src_offsets and dst_offsets are all in host memory or all in device
 * memory on the blocks' device (a mix is FEC_EINVAL); pattern_of is
 * independently host or device memory, as in fec_repair_batch.  Host arrays
 * are copied when the call is made; device arrays are read where they are, in
 * stream order, and nothing synchronises the stream.
 *
 * A stripe with sizes[s] > 0 FITS when offset + (rows - 1)*B + sizes[s] <=
 * bytes holds on both sides, evaluated without wrapping, rows being k for src
 * and ntargets for dst: the place of a FEC_REPAIR_NONE row must exist although
 * it is not written.  With host descriptor arrays a stripe that does not fit
 * is FEC_EINVAL, the message naming the stripe and the side; a host-side id >=
 * npatterns is FEC_EINVAL, naming the stripe.  With device arrays the kernel
 * makes both tests per stripe: a stripe that does not fit, or whose id is >=
 * npatterns, is neither read nor written, and no error is reported -- the rule
 * of the other writing ragged calls and of fec_repair_batch.
 *
 * Checked in this order, each FEC_EINVAL with a message naming the call:
 * fec_repair_batch's checks of the code and the pattern arguments, in its
 * order; a NULL sizes, src_offsets or dst_offsets; nstripes >= 2^32;
 * descriptor arrays of mixed memory kinds; a host-side id out of range; with
 * host arrays a stripe that does not fit.  Then FEC_ENODEV when no GPU is
 * visible.  nstripes == 0 returns FEC_OK.  A batch whose sizes are all zero,
 * or whose targets are all FEC_REPAIR_NONE, launches nothing.  src and dst are
 * device memory on one device or page-locked host memory; pageable memory
 * returns FEC_EINVAL.  The call stages per call, so it returns FEC_EINVAL while
 * the stream is being captured into a graph.  dst must not overlap src.
 *
 * k <= 4 runs matrepair_ragged<k,r>: matapply_ragged's walk with
 * matrepair_mixed's per-stripe record, one launch per 8 targets, a group of 8
 * no pattern uses skipped.  Wider codes are cut into runs of consecutive
 * stripes of one size and one pattern id whose two offsets each advance by a
 * constant, each run one shared-matrix launch of that pattern's used rows (at
 * worst one launch per stripe); device-side arrays are first copied to the
 * host there, which SYNCHRONISES the stream, and stripes that do not fit or
 * have a bad id are skipped. */
int fec_repair_batch_ragged(const fec_t* code,
                            const gf* src, size_t src_bytes, size_t src_block_stride,
                            const unsigned long long* src_offsets,
                            gf* dst, size_t dst_bytes, size_t dst_block_stride,
                            const unsigned long long* dst_offsets,
                            const unsigned long long* sizes,
                            const unsigned* present, const unsigned* targets, size_t ntargets,
                            size_t npatterns, const unsigned* pattern_of,
                            size_t nstripes, void* stream, unsigned flags);

/* Ragged parity update: fec_update_batch over stripes that each have their own
 * size, in one launch.  The arithmetic is fec_update_batch's, the layout
 * fec_repair_batch_ragged's.
 *
 * Input slot c of stripe s starts at newb + in_offsets[s] + c*B, with B =
 * in_block_stride, or sizes[s] when the stride is 0, and at the same offset in
 * oldb; with oldb == NULL newb holds the deltas old ^ new themselves.  Row i of
 * stripe s starts at rows + row_offsets[s] + i*B', B' formed the same way from
 * row_block_stride, and holds block block_nums[i]: num_block_nums distinct
 * numbers < n (host memory), in any order, primaries allowed.  Offsets are
 * arbitrary bytes.  A zero-size stripe is neither read nor written.
 *
 * changed: nstripes x nchanged numbers (unsigned, 4 bytes each), 1 <= nchanged
 * <= 4: word [s*nchanged + c] is the number of the primary input slot c of
 * stripe s carries, or FEC_UPDATE_NONE.  Every live slot contributes
 * E[block_nums[i]][j] . d to row i, IN PLACE; the same number in two slots
 * contributes twice.  A FEC_UPDATE_NONE slot is not read.  A row whose
 * coefficients for the stripe's live slots are all zero is neither read nor
 * written, and a stripe with no live slot is untouched.  The bytes are those of
 * fec_update_batch called once per stripe with nstripes = 1 and sz = sizes[s].
 *
 * sizes, in_offsets and row_offsets are all in host memory or all in device
 * memory on the blocks' device (a mix is FEC_EINVAL); changed is independently
 * host or device memory, as pattern_of is in fec_repair_batch_ragged.  Host
 * arrays are copied when the call is made; device arrays are read where they
 * are, in stream order.  NOTHING synchronises the stream, for any code.
 *
 * A stripe with sizes[s] > 0 FITS when offset + (slots - 1)*B + sizes[s] <=
 * bytes holds on both sides, evaluated without wrapping, slots being nchanged
 * for the inputs (oldb and newb are two arenas of in_bytes each) and
 * num_block_nums for the rows: the place of a FEC_UPDATE_NONE slot must exist
 * although it is not read, the rule FEC_REPAIR_NONE rows follow.  With host
 * descriptor arrays a stripe that does not fit is FEC_EINVAL, the message
 * naming the stripe and the side (the inputs / the rows).  A host-side number
 * that is neither < k nor FEC_UPDATE_NONE is FEC_EINVAL, naming the stripe and
 * the slot.  With device arrays the kernel makes both tests: a stripe that does
 * not fit is neither read nor written, a bad device-side number makes its slot
 * a FEC_UPDATE_NONE, and no error is reported.
 *
 * Checked before any GPU work, in this order, each FEC_EINVAL with a message
 * naming the call: fec_update_batch's checks in its order (invalid fec_t; NULL
 * newb, rows, block_nums or changed; num_block_nums == 0 or > n; a block number
 * >= n; a duplicate block number; nchanged == 0 or > 4); a NULL sizes,
 * in_offsets or row_offsets; nstripes >= 2^32; descriptor arrays of mixed
 * memory kinds; a bad number in a HOST-side changed; with host arrays a stripe
 * that does not fit.  Then FEC_ENODEV when no GPU is visible.  nstripes == 0
 * returns FEC_OK.  A batch whose sizes are all zero launches nothing (host
 * arrays).  oldb, newb and rows are device memory on one device or page-locked
 * host memory; pageable memory returns FEC_EINVAL.  The call stages per call,
 * so it returns FEC_EINVAL while the stream is being captured into a graph.
 * FEC_FLAG_ASYNC and FEC_FLAG_LIBRARY_STREAM as in fec_repair_batch_ragged;
 * FEC_FLAG_ROW_PADDING is accepted and ignored.  The rows of different stripes
 * must not overlap each other or the inputs: the result is then unspecified.
 *
 * Every code runs on matupdate_ragged<nchanged, r>: matupdate_reg's unit inside
 * matapply_ragged's walk.  One column of E per changed block is involved, so the
 * kernel does not depend on k, and no shape is cut into runs.  A launch takes
 * at most 8 rows; more run as row groups of 8 over one staging, each re-reading
 * the inputs.  The kernel XORs into the rows, so a block ends with its byte
 * tail, never with a last chunk shifted back over its neighbour. */
int fec_update_batch_ragged(const fec_t* code,
                            const gf* oldb, const gf* newb, size_t in_bytes, size_t in_block_stride,
                            const unsigned long long* in_offsets,
                            gf* rows, size_t row_bytes, size_t row_block_stride,
                            const unsigned long long* row_offsets,
                            const unsigned long long* sizes,
                            const unsigned* block_nums, size_t num_block_nums,
                            const unsigned* changed, size_t nchanged,
                            size_t nstripes, void* stream, unsigned flags);

/* Ragged in-place correction: fec_correct_batch over stripes that each have
 * their own size.  The arguments are exactly fec_locate_batch_ragged's, with
 * the arena writable.
 *
 * culprit[s] is the verdict fec_locate_batch_ragged gives for the blocks as
 * they were on entry, FEC_LOCATE_UNFIT included.  For a verdict h < nb the
 * sizes[s] bytes of slot h are rewritten by row h of fec_correct_rows from
 * slots 0..k-1, check 0 standing in for h when h < k.  Nothing else in caller
 * memory is written: no byte of a CLEAN, MANY, UNKNOWN, UNFIT or zero-size
 * stripe, no other slot of a corrected stripe, no byte past sizes[s] of slot h
 * (in a packed object that byte belongs to slot h + 1 or to the next stripe).
 * The guarantees are fec_correct_batch's.
 *
 * Memory kinds, result words in host or device memory, flags, capture and the
 * validation order are fec_locate_batch_ragged's, the messages naming this
 * call.  The location runs exactly as there; for k <= 4 and at most 8 checks
 * matcorrect_ragged<k> follows in the same stream over the verdict words in
 * device memory and the descriptors the location staged, a clean stripe costing
 * it scalar loads only, and it makes its own fit test.  For the shapes the
 * ragged location cuts into runs, each run's location is followed by the
 * uniform correction over that run's verdict words.  fec_last_kernel_name()
 * names the correction kernel where one ran. */
int fec_correct_batch_ragged(const fec_t* code,
                             gf* blocks, size_t bytes, size_t block_stride,
                             const unsigned long long* offsets,
                             const unsigned long long* sizes,
                             const unsigned* block_nums, size_t num_block_nums,
                             size_t nstripes,
                             unsigned* culprit, void* stream, unsigned flags);

/* Ragged pair location and correction: fec_locate2_batch / fec_correct2_batch
 * over stripes that each have their own size.  The arguments, their checks and
 * the order of the checks are fec_locate_batch_ragged's /
 * fec_correct_batch_ragged's, the messages naming these calls.  culprit holds
 * two planes as in fec_locate2_batch: words s and nstripes + s belong to
 * stripe s, 2 * nstripes words in all.
 *
 * Per stripe:
 *   - stripe s gets the two words fec_locate2_batch gives for that stripe alone
 *     with sz = sizes[s]: rules 1-4 with FEC_LOCATE_NONE in plane 1, and the
 *     pair (a, b) where rule 5 applies (c >= 4 and nb <= 32).  Outside that the
 *     words are (fec_locate_batch_ragged's verdict, FEC_LOCATE_NONE) and no
 *     error is returned;
 *   - a zero-size stripe is (FEC_LOCATE_CLEAN, FEC_LOCATE_NONE), neither read
 *     nor written;
 *   - with descriptor arrays in device memory a stripe that does not fit the
 *     arena is neither read nor written and gets (FEC_LOCATE_UNFIT,
 *     FEC_LOCATE_NONE); with host-side arrays it is FEC_EINVAL.
 * fec_correct2_batch_ragged returns the verdicts of the blocks as they were on
 * entry.  A single-slot verdict is healed exactly as fec_correct_batch_ragged
 * heals it; for a pair (a, b) the sizes[s] bytes of slots a and b are rewritten
 * from the k lowest other slots by fec_correct2_rows' rows.  Nothing else in
 * caller memory is written: no byte of a CLEAN, MANY, UNKNOWN, UNFIT or
 * zero-size stripe, no other slot of a healed stripe, no byte past sizes[s] of
 * a rewritten slot (in a packed object that byte is the next slot's or the
 * next stripe's).
 *
 * Memory kinds, culprit in device memory (in place, FEC_FLAG_ASYNC honoured) or
 * host memory (gathered and copied back, synchronous), page-locked arenas,
 * capture (FEC_EINVAL) and nstripes == 0 (FEC_OK) are the siblings'.
 *
 * For k <= 4 and 4 <= c <= 8 everything runs in the caller's stream and the
 * host reads neither a verdict nor the list: the ragged location
 * (matlocate_ragged<k,c>) with its descriptors staged and kept;
 * locate2_finish, which writes both planes and the dirty list; ragged_unfit
 * (device-side descriptors) over plane 0; (correct) matcorrect_ragged<k> for
 * the single slots; then pairs_locate_ragged, pairs_finish and (correct)
 * pairs_correct_ragged over the list, each listed stripe's size and offset
 * read by scalar loads and each kernel making its own fit test.  With k <= 4
 * and c < 4 the single-block ragged call runs and plane 1 is filled with NONE.
 * The other shapes (k > 4 or c > 8) are cut into runs of equal consecutive
 * stripes as fec_locate_batch_ragged cuts them, each run one fec_locate2_batch
 * / fec_correct2_batch into the whole call's planes.  fec_last_kernel_name()
 * is pairs_locate_ragged / pairs_correct_ragged where the ragged pair pass
 * ran, else what the single-block ragged call (or the run's uniform call)
 * reports. */
int fec_locate2_batch_ragged(const fec_t* code,
                             const gf* src, size_t src_bytes, size_t src_block_stride,
                             const unsigned long long* src_offsets,
                             const unsigned long long* sizes,
                             const unsigned* block_nums, size_t num_block_nums,
                             size_t nstripes,
                             unsigned* culprit, void* stream, unsigned flags);
int fec_correct2_batch_ragged(const fec_t* code,
                              gf* blocks, size_t bytes, size_t block_stride,
                              const unsigned long long* offsets,
                              const unsigned long long* sizes,
                              const unsigned* block_nums, size_t num_block_nums,
                              size_t nstripes,
                              unsigned* culprit, void* stream, unsigned flags);

/* Batched calls over several GPUs of this process.  The nstripes stripes are
 * split into contiguous, balanced ranges, one per entry of devices[] (entry d
 * gets stripes [d*q + min(d, e), ...), q = nstripes / ndevices, e = the
 * remainder: zfec_amd.shard.shard_range), and every range runs on its device
 * from a persistent host thread of the library bound to that device, with its
 * own stream and pinned staging slots; the call returns when all are done.
 * src / dst must be host memory (pageable: staged per device; page-locked:
 * read and written in place), each GPU moving its share over its own PCIe
 * link.  A device may be listed more than once (several threads on one GPU).
 * Layout, block numbers and flags as fec_encode_batch / fec_decode_batch
 * (FEC_FLAG_ASYNC and FEC_FLAG_LIBRARY_STREAM do not apply: the call is
 * synchronous on the library's streams).  The first failing range's status
 * is returned, its message prefixed with the device. */
int fec_encode_batch_multi(const fec_t* code,
                           const gf* src, size_t src_block_stride, size_t src_stripe_stride,
                           gf* dst, size_t dst_block_stride, size_t dst_stripe_stride,
                           const unsigned* block_nums, size_t num_block_nums, size_t sz, size_t nstripes,
                           const int* devices, size_t ndevices, unsigned flags);
int fec_decode_batch_multi(const fec_t* code,
                           const gf* src, size_t src_block_stride, size_t src_stripe_stride,
                           gf* dst, size_t dst_block_stride, size_t dst_stripe_stride,
                           const unsigned* index, size_t sz, size_t nstripes,
                           const int* devices, size_t ndevices, unsigned flags);

/* Several batched calls in one: job i is exactly the fec_encode_batch
 * (kind FEC_JOB_ENCODE: nums = block_nums, num_nums entries) or
 * fec_decode_batch (kind FEC_JOB_DECODE: nums = index, k entries; num_nums
 * ignored) call its fields describe, with its own flags (only
 * FEC_FLAG_ROW_PADDING and FEC_FLAG_ALL_PRIMARIES apply per job).  The jobs
 * are independent: they may run concurrently and in any order, so no job may
 * read or write a buffer another job writes.  Two consecutive jobs on one
 * device, over codes with the same k and of register-kernel shape (k <= 4,
 * at most 8 outputs each, the narrower job at most k outputs; blocks longer
 * than 4 KiB or fewer than 64 stripes) share ONE launch, which pays one launch
 * ramp-up and drain instead of two (a stripe's encode next to another
 * stripe's decode); other jobs launch one at a time on the same stream.
 * `stream` and `flags` (FEC_FLAG_ASYNC, FEC_FLAG_LIBRARY_STREAM) apply to the
 * whole call.  The first failing job's status is returned, its message
 * prefixed "job i".  (An extension: zfec/fec.h has no batched calls.)  On the
 * cfg2 step (a 64 MiB K=3/M=10 stripe's encode and another's decode) one
 * paired launch per step measured 2465-2514 GB/s against 2506-2529 for the
 * two launches on two streams and about 2350 on one stream
 * (profiles/r03_pair_ab.json). */
#define FEC_JOB_ENCODE 0u
#define FEC_JOB_DECODE 1u
typedef struct fec_batch_job {
    const fec_t* code;
    unsigned kind;
    unsigned flags;
    const gf* src;
    size_t src_block_stride, src_stripe_stride;
    gf* dst;
    size_t dst_block_stride, dst_stripe_stride;
    const unsigned* nums;
    size_t num_nums;
    size_t sz, nstripes;
} fec_batch_job;
int fec_run_batch_jobs(const fec_batch_job* jobs, size_t njobs, void* stream, unsigned flags);

/* Page-locked host memory (hipHostMalloc): host buffers passed to fec_encode /
 * fec_decode from here are read and written by the kernel in place (no
 * per-call pinning, no staging copies).  NULL on failure (status set). */
void* fec_host_alloc(size_t bytes);
void fec_host_free(void* p);

/* Number of visible GPUs (0 when none; never aborts). */
int fec_device_count(void);

/* Library version string. */
const char* fec_version(void);

/* Name of the table-kernel variant a launch with k inputs and r outputs uses
 * when no run-time specialised kernel applies (diagnostics and profiling;
 * k <= 32, r <= 48 per launch). */
const char* fec_kernel_name(unsigned k, unsigned r);

/* Name of the kernel the calling thread launched last. */
const char* fec_last_kernel_name(void);

/* Run-time specialised bit-sliced kernels (hipRTC; zfec_amd/csrc/bitslice.cpp):
 * the coefficient matrix of a launch compiled into the instruction stream.
 * mode 0 = off; 1 = auto (default; launches of >= 8 MiB of wide codes: a
 * matrix's second such launch queues its compile in a background thread while
 * the table kernels serve; kernels are cached in memory and in jit_cache/ next
 * to the library, at most 512); 2 = force (every launch with blocks of
 * >= 2048 bytes, compiled synchronously).  The environment variable
 * ZFEC_HIP_JIT=0|auto|force sets the initial mode.  Returns the previous
 * mode; any other value of `mode` only queries.  Results are bit-identical in
 * every mode. */
int fec_jit_mode(int mode);

/* Wide-code launches that no compiled specialised kernel serves (a decode of
 * an erasure pattern seen for the first time, small launches, JIT off) run on
 * the bit-sliced kernels that take the coefficient matrix as run-time data (no
 * compile step): mode 2 = matapply_bsr (default; the specialised kernels'
 * instruction stream, one call per coefficient, any k, r up to 256/256);
 * 1 = matapply_bsg only; 0 = off (the table-lookup
 * kernels serve them; environment ZFEC_HIP_GENERIC=0 / 1 / 2 starts in that
 * mode).  Returns the previous mode; any other value only queries.  Results are
 * bit-identical in every mode. */
int fec_generic_mode(int mode);

/* Wait for background compiles; returns the number of compiled kernels. */
int fec_jit_wait(void);

/* Diagnostics and A/B runs.  The ZFEC_HIP_* environment knobs are read once,
 * at the library's first call; fec_reload_config re-reads them (returns
 * FEC_OK).  fec_last_wait: how the calling thread's last synchronous
 * small-object call waited for its kernel -- 1 = on the completion word the
 * kernel itself wrote to pinned host memory, 0 = hipStreamSynchronize. */
int fec_reload_config(void);
int fec_last_wait(void);

/* Compile now (no GPU needed) the kernels an fec_encode of block_nums, or an
 * fec_decode from `index` (flags as fec_decode_ex), would use.  FEC_OK, or
 * FEC_EHIP with the compiler's message. */
int fec_jit_prepare_encode(const fec_t* code, const unsigned* block_nums, size_t num_block_nums);
int fec_jit_prepare_decode(const fec_t* code, const unsigned* index, unsigned flags);

#ifdef __cplusplus
}
#endif

#endif /* ZFEC_HIP_H */
