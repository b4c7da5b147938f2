// ragged_repair_validate.cpp -- the validation path of fec_repair_batch_ragged
// and fec_correct_batch_ragged under AddressSanitizer and
// UndefinedBehaviorSanitizer (make asan-repair: every host object of
// libzfec_hip.so compiled with both and linked into this program).  Runs
// without a GPU: every check the header lists comes before any GPU work, so
// what is exercised is the argument checks in their order, the fit test with
// its wrap cases, the message formatting, and the end a valid call meets on a
// machine without a GPU (FEC_ENODEV) or with one (the pageable arena refused).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/zfec_hip.h"

namespace {

int g_fail = 0;

#define CHECK(c)                                                                          \
    do {                                                                                  \
        if (!(c)) {                                                                       \
            fprintf(stderr, "CHECK failed %s:%d: %s [%s]\n", __FILE__, __LINE__, #c,      \
                    fec_last_error_message());                                            \
            ++g_fail;                                                                     \
        }                                                                                 \
    } while (0)

bool says(const char* needle) { return std::strstr(fec_last_error_message(), needle) != nullptr; }

typedef unsigned long long u64;

void repair() {
    const char* const name = "fec_repair_batch_ragged";
    fec_t* code = fec_new(3, 10);
    CHECK(code != nullptr);
    // two patterns of K=3/M=10, two targets each; three stripes, the middle one empty
    const unsigned present[6] = {7, 0, 4, 9, 8, 3}, targets[4] = {1, FEC_REPAIR_NONE, 0, 2}, ids[3] = {0, 1, 1};
    const u64 sizes[3] = {8, 0, 24}, soff[3] = {0, 24, 24}, doff[3] = {0, 16, 16};
    std::vector<gf> src(3 * 32), dst(2 * 32, 0x55);
    const size_t sb = src.size(), db = dst.size();
    const auto call = [&](const fec_t* c, const gf* s, gf* d, const u64* so, const u64* dof, const u64* sz,
                          const unsigned* pr, const unsigned* tg, size_t nt, size_t np, const unsigned* po,
                          size_t ns, size_t sbytes, size_t dbytes, size_t sbs = 0, size_t dbs = 0) {
        return fec_repair_batch_ragged(c, s, sbytes, sbs, so, d, dbytes, dbs, dof, sz, pr, tg, nt, np, po, ns, nullptr,
                                       0);
    };
    // 1. fec_repair_batch's checks of the code and the pattern arguments, in its order
    CHECK(call(nullptr, nullptr, nullptr, soff, doff, sizes, present, targets, 2, 2, ids, 3, sb, db) == FEC_EINVAL);
    CHECK(says(name) && says("invalid fec_t"));
    CHECK(call(code, nullptr, dst.data(), soff, doff, sizes, nullptr, targets, 2, 2, ids, 3, sb, db) == FEC_EINVAL);
    CHECK(says(name) && says("NULL buffer"));
    CHECK(call(code, src.data(), dst.data(), soff, doff, sizes, nullptr, nullptr, 2, 2, ids, 3, sb, db) == FEC_EINVAL);
    CHECK(says("present is NULL"));
    CHECK(call(code, src.data(), dst.data(), soff, doff, sizes, present, nullptr, 0, 2, ids, 3, sb, db) == FEC_EINVAL);
    CHECK(says("targets is NULL"));
    CHECK(call(code, src.data(), dst.data(), soff, doff, sizes, present, targets, 0, 0, ids, 3, sb, db) == FEC_EINVAL);
    CHECK(says(name) && says("ntargets is 0"));
    CHECK(call(code, src.data(), dst.data(), soff, doff, sizes, present, targets, 33, 2, ids, 3, sb, db) == FEC_EINVAL);
    CHECK(says("ntargets is 33"));
    CHECK(call(code, src.data(), dst.data(), soff, doff, sizes, present, targets, 2, 0, ids, 3, sb, db) == FEC_EINVAL);
    CHECK(says("npatterns is 0"));
    CHECK(call(code, src.data(), dst.data(), soff, doff, sizes, present, targets, 2, 65537, nullptr, 3, sb, db) ==
          FEC_EINVAL);
    CHECK(says("65537 patterns"));
    CHECK(call(code, src.data(), dst.data(), soff, doff, sizes, present, targets, 2, 2, nullptr, 3, sb, db) ==
          FEC_EINVAL);
    CHECK(says(name) && says("pattern_of is NULL with 2 patterns"));
    const unsigned far[6] = {7, 0, 10, 9, 9, 3}, twice[6] = {7, 0, 4, 9, 9, 3}, bad_t[4] = {1, 10, 0, 2};
    CHECK(call(code, src.data(), dst.data(), soff, doff, sizes, far, bad_t, 2, 2, ids, 3, sb, db) == FEC_EINVAL);
    CHECK(says("pattern 0: block number 10 out of range"));
    CHECK(call(code, src.data(), dst.data(), soff, doff, sizes, twice, bad_t, 2, 2, ids, 3, sb, db) == FEC_EINVAL);
    CHECK(says("pattern 1: duplicate block number 9"));
    CHECK(call(code, src.data(), dst.data(), soff, doff, sizes, present, bad_t, 2, 2, ids, 3, sb, db) == FEC_EINVAL);
    CHECK(says(name) && says("pattern 0: target 10"));
    // 2. the descriptor arrays, after the patterns
    CHECK(call(code, src.data(), dst.data(), nullptr, nullptr, nullptr, present, bad_t, 2, 2, ids, 3, sb, db) ==
          FEC_EINVAL);
    CHECK(says("target 10"));
    CHECK(call(code, src.data(), dst.data(), nullptr, nullptr, nullptr, present, targets, 2, 2, ids, 3, sb, db) ==
          FEC_EINVAL);
    CHECK(says(name) && says("sizes is NULL"));
    CHECK(call(code, src.data(), dst.data(), nullptr, nullptr, sizes, present, targets, 2, 2, ids, 3, sb, db) ==
          FEC_EINVAL);
    CHECK(says("src_offsets is NULL"));
    CHECK(call(code, src.data(), dst.data(), soff, nullptr, sizes, present, targets, 2, 2, ids, 3, sb, db) ==
          FEC_EINVAL);
    CHECK(says("dst_offsets is NULL"));
    CHECK(call(code, src.data(), dst.data(), soff, doff, sizes, present, targets, 2, 2, ids, 0, sb, db) == FEC_OK);
    // 3. the stripe count, before any array is read (the arrays hold three words)
    CHECK(call(code, src.data(), dst.data(), soff, doff, sizes, present, targets, 2, 2, ids, size_t(1) << 32, sb,
               db) == FEC_EINVAL);
    CHECK(says(name) && says("fewer than 2^32"));
    // 5. a host-side id out of range comes before the fit
    const unsigned bad_ids[3] = {0, 2, 1};
    const u64 late[3] = {0, 24, 25};
    CHECK(call(code, src.data(), dst.data(), late, doff, sizes, present, targets, 2, 2, bad_ids, 3, sb, db) ==
          FEC_EINVAL);
    CHECK(says(name) && says("stripe 1: pattern id 2 out of range (npatterns = 2)"));
    // 6. the fit of host-side descriptors, on both sides; the side is named
    CHECK(call(code, src.data(), dst.data(), late, doff, sizes, present, targets, 2, 2, ids, 3, sb, db) == FEC_EINVAL);
    CHECK(says(name) && says("stripe 2 does not fit src"));
    CHECK(call(code, src.data(), dst.data(), soff, doff, sizes, present, targets, 2, 2, ids, 3, sb - 1, db) ==
          FEC_EINVAL);
    CHECK(says("stripe 2 does not fit src"));
    const u64 dlate[3] = {0, 16, 17};
    CHECK(call(code, src.data(), dst.data(), soff, dlate, sizes, present, targets, 2, 2, ids, 3, sb, db) ==
          FEC_EINVAL);
    CHECK(says("stripe 2 does not fit dst"));
    // the place of a FEC_REPAIR_NONE row must exist: row 1 of stripe 0 is one, and dst ends inside it
    const u64 one[1] = {16}, zero[1] = {0}, wrap[1] = {~0ull - 7};
    const unsigned p0[3] = {7, 0, 4}, t0[2] = {1, FEC_REPAIR_NONE};
    CHECK(call(code, src.data(), dst.data(), zero, zero, one, p0, t0, 2, 1, nullptr, 1, sb, 31) == FEC_EINVAL);
    CHECK(says("stripe 0 does not fit dst"));
    // wraps of 2^64: offset + size, (rows - 1) * stride
    CHECK(call(code, src.data(), dst.data(), wrap, zero, one, p0, t0, 2, 1, nullptr, 1, sb, db) == FEC_EINVAL);
    CHECK(says("stripe 0 does not fit src"));
    CHECK(call(code, src.data(), dst.data(), zero, wrap, one, p0, t0, 2, 1, nullptr, 1, sb, db) == FEC_EINVAL);
    CHECK(says("stripe 0 does not fit dst"));
    CHECK(call(code, src.data(), dst.data(), zero, zero, one, p0, t0, 2, 1, nullptr, 1, ~size_t(0), db,
               size_t(1) << 63) == FEC_EINVAL);
    CHECK(says("stripe 0 does not fit src"));
    CHECK(call(code, src.data(), dst.data(), zero, zero, one, p0, t0, 2, 1, nullptr, 1, sb, ~size_t(0), 0,
               ~size_t(0)) == FEC_EINVAL);
    CHECK(says("stripe 0 does not fit dst"));
    // a zero-size stripe is not looked at, wherever its offsets point
    const u64 wild[3] = {0, 1ull << 63, 24}, dwild[3] = {0, 1ull << 63, 16};
    int st = call(code, src.data(), dst.data(), wild, dwild, sizes, present, targets, 2, 2, ids, 3, sb, db);
    CHECK(!says("does not fit"));
    // 7. a valid call: no GPU here, or the pageable arena refused; never an output byte written before that
    st = call(code, src.data(), dst.data(), soff, doff, sizes, present, targets, 2, 2, ids, 3, sb, db);
    CHECK(st == FEC_ENODEV || (st == FEC_EINVAL && says(name) && says("pageable host memory")));
    st = call(code, src.data(), dst.data(), zero, zero, one, p0, t0, 2, 1, nullptr, 1, sb, db);
    CHECK(st == FEC_ENODEV || (st == FEC_EINVAL && says("pageable host memory")));
    for (gf b : dst) CHECK(b == 0x55);
    fec_free(code);
}

void correct() {
    const char* const name = "fec_correct_batch_ragged";
    fec_t* code = fec_new(3, 10);
    CHECK(code != nullptr);
    const unsigned nums[7] = {7, 0, 4, 1, 9, 2, 5};
    const u64 sizes[3] = {8, 0, 24}, offs[3] = {0, 56, 56};
    std::vector<gf> arena(7 * 32, 0x3C);
    unsigned res[3] = {0x55, 0x55, 0x55};
    const size_t bytes = arena.size();
    const auto fn = fec_correct_batch_ragged;

    CHECK(fn(nullptr, arena.data(), bytes, 0, offs, sizes, nums, 7, 3, res, nullptr, 0) == FEC_EINVAL);
    CHECK(says(name) && says("invalid fec_t"));
    CHECK(fn(code, nullptr, bytes, 0, offs, sizes, nums, 7, 3, res, nullptr, 0) == FEC_EINVAL);
    CHECK(says(name) && says("blocks is NULL"));
    CHECK(fn(code, arena.data(), bytes, 0, offs, nullptr, nums, 7, 3, res, nullptr, 0) == FEC_EINVAL);
    CHECK(says("sizes is NULL"));
    CHECK(fn(code, arena.data(), bytes, 0, nullptr, sizes, nums, 7, 3, res, nullptr, 0) == FEC_EINVAL);
    CHECK(says("offsets is NULL"));
    CHECK(fn(code, arena.data(), bytes, 0, offs, sizes, nullptr, 7, 3, res, nullptr, 0) == FEC_EINVAL);
    CHECK(says("block_nums is NULL"));
    CHECK(fn(code, arena.data(), bytes, 0, offs, sizes, nums, 7, 3, nullptr, nullptr, 0) == FEC_EINVAL);
    CHECK(says("culprit is NULL"));
    CHECK(fn(code, arena.data(), bytes, 0, offs, sizes, nums, 3, 3, res, nullptr, 0) == FEC_EINVAL);
    CHECK(says(name) && says("nothing to check"));
    const unsigned many[11] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 12};
    CHECK(fn(code, arena.data(), bytes, 0, offs, sizes, many, 11, 3, res, nullptr, 0) == FEC_EINVAL);
    CHECK(says("only n = 10"));
    const unsigned far[4] = {5, 5, 1, 10}, twice[4] = {5, 5, 1, 9};
    CHECK(fn(code, arena.data(), bytes, 0, offs, sizes, far, 4, 3, res, nullptr, 0) == FEC_EINVAL);
    CHECK(says("block number 10 out of range"));
    CHECK(fn(code, arena.data(), bytes, 0, offs, sizes, twice, 4, 3, res, nullptr, 0) == FEC_EINVAL);
    CHECK(says("duplicate block number 5"));
    CHECK(fn(code, arena.data(), bytes, 0, offs, sizes, nums, 7, size_t(1) << 32, res, nullptr, 0) == FEC_EINVAL);
    CHECK(says(name) && says("fewer than 2^32"));
    CHECK(fn(code, arena.data(), bytes, 0, offs, sizes, nums, 7, 0, res, nullptr, 0) == FEC_OK);
    const u64 late[3] = {0, 56, 57};
    CHECK(fn(code, arena.data(), bytes, 0, late, sizes, nums, 7, 3, res, nullptr, 0) == FEC_EINVAL);
    CHECK(says(name) && says("stripe 2 does not fit blocks"));
    CHECK(fn(code, arena.data(), bytes - 1, 0, offs, sizes, nums, 7, 3, res, nullptr, 0) == FEC_EINVAL);
    CHECK(says("stripe 2 does not fit blocks"));
    const u64 one[1] = {16}, wrap[1] = {~0ull - 7}, zero[1] = {0};
    CHECK(fn(code, arena.data(), bytes, 0, wrap, one, nums, 7, 1, res, nullptr, 0) == FEC_EINVAL);
    CHECK(says("stripe 0 does not fit blocks"));
    CHECK(fn(code, arena.data(), ~size_t(0), size_t(1) << 63, zero, one, nums, 7, 1, res, nullptr, 0) == FEC_EINVAL);
    CHECK(says("stripe 0 does not fit blocks"));
    CHECK(fn(code, arena.data(), 6 * 30 + 15, 30, zero, one, nums, 7, 1, res, nullptr, 0) == FEC_EINVAL);
    const u64 wild[3] = {0, 1ull << 63, 56};
    int st = fn(code, arena.data(), bytes, 0, wild, sizes, nums, 7, 3, res, nullptr, 0);
    CHECK(!says("does not fit"));
    st = fn(code, arena.data(), bytes, 0, offs, sizes, nums, 7, 3, res, nullptr, FEC_FLAG_ROW_PADDING);
    CHECK(st == FEC_ENODEV || (st == FEC_EINVAL && says(name) && says("blocks is pageable host memory")));
    CHECK(res[0] == 0x55 && res[1] == 0x55 && res[2] == 0x55);
    for (gf b : arena) CHECK(b == 0x3C);
    fec_free(code);
}

}  // namespace

int main() {
    fec_init();
    repair();
    correct();
    if (g_fail) {
        fprintf(stderr, "ragged_repair_validate: %d check(s) failed\n", g_fail);
        return 1;
    }
    printf("ragged_repair_validate: ok\n");
    return 0;
}
