// ragged_update_validate.cpp -- the validation path of fec_update_batch_ragged
// under AddressSanitizer and UndefinedBehaviorSanitizer (make asan-update:
// every host object of libzfec_hip.so compiled with both and linked into this
// program).  Runs without a GPU: every check the header lists comes before any
// GPU work, so what is exercised is the argument checks in their order, the fit
// test with its wrap cases on both sides, the message formatting, and the end a
// valid call meets on a machine without a GPU (FEC_ENODEV) or with one (the
// pageable arena refused).
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

void update() {
    const char* const name = "fec_update_batch_ragged";
    fec_t* code = fec_new(3, 10);
    CHECK(code != nullptr);
    // K=3/M=10, two stored rows, two slots per stripe; three stripes, the middle one empty
    const unsigned nums[2] = {7, 4}, changed[6] = {0, FEC_UPDATE_NONE, 1, 1, 2, 0};
    const u64 sizes[3] = {8, 0, 24}, ioff[3] = {0, 16, 16}, roff[3] = {0, 16, 16};
    std::vector<gf> oldb(2 * 32, 0x11), newb(2 * 32, 0x22), rows(2 * 32, 0x55);
    const size_t ib = newb.size(), rb = rows.size();
    const auto call = [&](const fec_t* c, const gf* o, const gf* n, gf* r, const u64* io, const u64* ro, const u64* sz,
                          const unsigned* bn, size_t nbn, const unsigned* ch, size_t nc, size_t ns, size_t ibytes,
                          size_t rbytes, size_t ibs = 0, size_t rbs = 0, unsigned flags = 0) {
        return fec_update_batch_ragged(c, o, n, ibytes, ibs, io, r, rbytes, rbs, ro, sz, bn, nbn, ch, nc, ns, nullptr,
                                       flags);
    };
    gf* const R = rows.data();
    const gf *const O = oldb.data(), *const N = newb.data();
    // 1. fec_update_batch's checks, in its order
    CHECK(call(nullptr, O, nullptr, nullptr, ioff, roff, sizes, nums, 2, changed, 2, 3, ib, rb) == FEC_EINVAL);
    CHECK(says(name) && says("invalid fec_t"));
    CHECK(call(code, O, nullptr, nullptr, ioff, roff, sizes, nullptr, 2, nullptr, 2, 3, ib, rb) == FEC_EINVAL);
    CHECK(says(name) && says("newb is NULL"));
    CHECK(call(code, O, N, nullptr, ioff, roff, sizes, nullptr, 2, nullptr, 2, 3, ib, rb) == FEC_EINVAL);
    CHECK(says("rows is NULL"));
    CHECK(call(code, O, N, R, ioff, roff, sizes, nullptr, 2, nullptr, 2, 3, ib, rb) == FEC_EINVAL);
    CHECK(says("block_nums is NULL"));
    CHECK(call(code, O, N, R, ioff, roff, sizes, nums, 0, nullptr, 2, 3, ib, rb) == FEC_EINVAL);
    CHECK(says("changed is NULL"));
    CHECK(call(code, O, N, R, ioff, roff, sizes, nums, 0, changed, 0, 3, ib, rb) == FEC_EINVAL);
    CHECK(says(name) && says("num_block_nums is 0"));
    const unsigned many[11] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12};
    CHECK(call(code, O, N, R, ioff, roff, sizes, many, 11, changed, 0, 3, ib, rb) == FEC_EINVAL);
    CHECK(says("num_block_nums is 11"));
    const unsigned far[2] = {7, 10}, twice[2] = {7, 7};
    CHECK(call(code, O, N, R, ioff, roff, sizes, far, 2, changed, 0, 3, ib, rb) == FEC_EINVAL);
    CHECK(says(name) && says("block number 10 out of range"));
    CHECK(call(code, O, N, R, ioff, roff, sizes, twice, 2, changed, 0, 3, ib, rb) == FEC_EINVAL);
    CHECK(says("duplicate block number 7"));
    CHECK(call(code, O, N, R, nullptr, nullptr, nullptr, nums, 2, changed, 0, 3, ib, rb) == FEC_EINVAL);
    CHECK(says(name) && says("nchanged is 0"));
    CHECK(call(code, O, N, R, nullptr, nullptr, nullptr, nums, 2, changed, 5, 3, ib, rb) == FEC_EINVAL);
    CHECK(says("nchanged is 5"));
    // 2. the descriptor arrays, after those
    CHECK(call(code, O, N, R, nullptr, nullptr, nullptr, nums, 2, changed, 2, 3, ib, rb) == FEC_EINVAL);
    CHECK(says(name) && says("sizes is NULL"));
    CHECK(call(code, O, N, R, nullptr, nullptr, sizes, nums, 2, changed, 2, 3, ib, rb) == FEC_EINVAL);
    CHECK(says("in_offsets is NULL"));
    CHECK(call(code, O, N, R, ioff, nullptr, sizes, nums, 2, changed, 2, 3, ib, rb) == FEC_EINVAL);
    CHECK(says("row_offsets is NULL"));
    CHECK(call(code, O, N, R, ioff, roff, sizes, nums, 2, changed, 2, 0, ib, rb) == FEC_OK);
    // 3. the stripe count, before any array is read (the arrays hold three words)
    CHECK(call(code, O, N, R, ioff, roff, sizes, nums, 2, changed, 2, size_t(1) << 32, ib, rb) == FEC_EINVAL);
    CHECK(says(name) && says("fewer than 2^32"));
    // 5. a bad host-side number comes before the fit; FEC_UPDATE_NONE is none
    const unsigned bad_ch[6] = {0, FEC_UPDATE_NONE, 1, 3, 2, 0};
    const u64 late[3] = {0, 16, 17};
    CHECK(call(code, O, N, R, late, roff, sizes, nums, 2, bad_ch, 2, 3, ib, rb) == FEC_EINVAL);
    CHECK(says(name) && says("stripe 1, slot 1: changed block 3 is neither a primary (k = 3) nor FEC_UPDATE_NONE"));
    // 6. the fit of host-side descriptors, on both sides; the side is named
    CHECK(call(code, O, N, R, late, roff, sizes, nums, 2, changed, 2, 3, ib, rb) == FEC_EINVAL);
    CHECK(says(name) && says("stripe 2 does not fit the inputs"));
    CHECK(call(code, nullptr, N, R, ioff, roff, sizes, nums, 2, changed, 2, 3, ib - 1, rb) == FEC_EINVAL);
    CHECK(says("stripe 2 does not fit the inputs"));
    CHECK(call(code, O, N, R, ioff, late, sizes, nums, 2, changed, 2, 3, ib, rb) == FEC_EINVAL);
    CHECK(says("stripe 2 does not fit the rows"));
    CHECK(call(code, O, N, R, ioff, roff, sizes, nums, 2, changed, 2, 3, ib, rb - 1) == FEC_EINVAL);
    CHECK(says("stripe 2 does not fit the rows"));
    // the place of a FEC_UPDATE_NONE slot must exist: slot 1 of stripe 0 is one, and the inputs end inside it
    const u64 one[1] = {16}, zero[1] = {0}, wrap[1] = {~0ull - 7};
    const unsigned ch0[2] = {0, FEC_UPDATE_NONE};
    CHECK(call(code, O, N, R, zero, zero, one, nums, 2, ch0, 2, 1, 31, rb) == FEC_EINVAL);
    CHECK(says("stripe 0 does not fit the inputs"));
    CHECK(call(code, O, N, R, zero, zero, one, nums, 2, ch0, 1, 1, 16, 32) != FEC_EINVAL || !says("does not fit"));
    // wraps of 2^64: offset + size, (slots - 1) * stride
    CHECK(call(code, O, N, R, wrap, zero, one, nums, 2, ch0, 2, 1, ib, rb) == FEC_EINVAL);
    CHECK(says("stripe 0 does not fit the inputs"));
    CHECK(call(code, O, N, R, zero, wrap, one, nums, 2, ch0, 2, 1, ib, rb) == FEC_EINVAL);
    CHECK(says("stripe 0 does not fit the rows"));
    const unsigned nums3[3] = {7, 4, 0}, ch3[3] = {0, FEC_UPDATE_NONE, 1};
    CHECK(call(code, O, N, R, zero, zero, one, nums, 2, ch3, 3, 1, ~size_t(0), rb, size_t(1) << 63) == FEC_EINVAL);
    CHECK(says("stripe 0 does not fit the inputs"));
    CHECK(call(code, O, N, R, zero, zero, one, nums3, 3, ch0, 2, 1, ib, ~size_t(0), 0, size_t(1) << 63) ==
          FEC_EINVAL);
    CHECK(says("stripe 0 does not fit the rows"));
    CHECK(call(code, O, N, R, zero, zero, one, nums, 2, ch0, 2, 1, ib, ~size_t(0), 0, ~size_t(0)) == FEC_EINVAL);
    CHECK(says("stripe 0 does not fit the rows"));
    // a zero-size stripe is not looked at, wherever its offsets point
    const u64 wild[3] = {0, 1ull << 63, 16};
    int st = call(code, O, N, R, wild, wild, sizes, nums, 2, changed, 2, 3, ib, rb);
    CHECK(!says("does not fit"));
    // 7. a valid call: no GPU here, or the pageable arena refused; never a row byte written before that
    st = call(code, O, N, R, ioff, roff, sizes, nums, 2, changed, 2, 3, ib, rb, 0, 0, FEC_FLAG_ROW_PADDING);
    CHECK(st == FEC_ENODEV || (st == FEC_EINVAL && says(name) && says("pageable host memory")));
    st = call(code, nullptr, N, R, zero, zero, one, nums, 2, ch0, 2, 1, ib, rb);
    CHECK(st == FEC_ENODEV || (st == FEC_EINVAL && says("pageable host memory")));
    for (gf b : rows) CHECK(b == 0x55);
    for (gf b : newb) CHECK(b == 0x22);
    fec_free(code);
}

}  // namespace

int main() {
    fec_init();
    update();
    if (g_fail) {
        fprintf(stderr, "ragged_update_validate: %d check(s) failed\n", g_fail);
        return 1;
    }
    printf("ragged_update_validate: ok\n");
    return 0;
}
