// ragged_scrub_validate.cpp -- the validation path of fec_verify_batch_ragged
// and fec_locate_batch_ragged under AddressSanitizer and
// UndefinedBehaviorSanitizer (make asan-scrub: every host object of
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

typedef int (*ScrubFn)(const fec_t*, const gf*, size_t, size_t, const unsigned long long*, const unsigned long long*,
                       const unsigned*, size_t, size_t, unsigned*, void*, unsigned);

bool says(const char* needle) { return std::strstr(fec_last_error_message(), needle) != nullptr; }

void run(ScrubFn fn, const char* name, const char* out_name) {
    fec_t* code = fec_new(3, 10);
    CHECK(code != nullptr);
    const unsigned nums[7] = {7, 0, 4, 1, 9, 2, 5};
    const unsigned long long sizes[3] = {8, 0, 24}, offs[3] = {0, 56, 56};
    std::vector<gf> arena(7 * 32);
    unsigned res[3] = {0x55, 0x55, 0x55};
    const size_t bytes = arena.size();

    CHECK(fn(nullptr, arena.data(), bytes, 0, offs, sizes, nums, 7, 3, res, nullptr, 0) == FEC_EINVAL);
    CHECK(says(name) && says("invalid fec_t"));
    CHECK(fn(code, nullptr, bytes, 0, offs, sizes, nums, 7, 3, res, nullptr, 0) == FEC_EINVAL && says("src is NULL"));
    CHECK(fn(code, arena.data(), bytes, 0, offs, nullptr, nums, 7, 3, res, nullptr, 0) == FEC_EINVAL);
    CHECK(says("sizes is NULL"));
    CHECK(fn(code, arena.data(), bytes, 0, nullptr, sizes, nums, 7, 3, res, nullptr, 0) == FEC_EINVAL);
    CHECK(says("src_offsets is NULL"));
    CHECK(fn(code, arena.data(), bytes, 0, offs, sizes, nullptr, 7, 3, res, nullptr, 0) == FEC_EINVAL);
    CHECK(says("block_nums is NULL"));
    CHECK(fn(code, arena.data(), bytes, 0, offs, sizes, nums, 7, 3, nullptr, nullptr, 0) == FEC_EINVAL);
    CHECK(says(out_name) && says("is NULL"));
    // the block numbers: too few, too many, out of range, a duplicate
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
    // the stripe count is refused before any array is read (the arrays hold three words)
    CHECK(fn(code, arena.data(), bytes, 0, offs, sizes, nums, 7, size_t(1) << 32, res, nullptr, 0) == FEC_EINVAL);
    CHECK(says("fewer than 2^32"));
    CHECK(fn(code, arena.data(), bytes, 0, offs, sizes, nums, 7, 0, res, nullptr, 0) == FEC_OK);
    // the fit of host-side descriptors: one byte too far, a short arena, wraps of 2^64, a fixed stride
    const unsigned long long late[3] = {0, 56, 57};
    CHECK(fn(code, arena.data(), bytes, 0, late, sizes, nums, 7, 3, res, nullptr, 0) == FEC_EINVAL);
    CHECK(says("stripe 2 does not fit src"));
    CHECK(fn(code, arena.data(), bytes - 1, 0, offs, sizes, nums, 7, 3, res, nullptr, 0) == FEC_EINVAL);
    CHECK(says("stripe 2 does not fit src"));
    const unsigned long long one[1] = {16}, wrap[1] = {~0ull - 7}, zero[1] = {0};
    CHECK(fn(code, arena.data(), bytes, 0, wrap, one, nums, 7, 1, res, nullptr, 0) == FEC_EINVAL);
    CHECK(says("stripe 0 does not fit src"));
    CHECK(fn(code, arena.data(), ~size_t(0), size_t(1) << 63, zero, one, nums, 7, 1, res, nullptr, 0) == FEC_EINVAL);
    CHECK(says("stripe 0 does not fit src"));
    CHECK(fn(code, arena.data(), 6 * 30 + 15, 30, zero, one, nums, 7, 1, res, nullptr, 0) == FEC_EINVAL);
    // a zero-size stripe is not looked at, wherever its offset points
    const unsigned long long wild[3] = {0, 1ull << 63, 56};
    int st = fn(code, arena.data(), bytes, 0, wild, sizes, nums, 7, 3, res, nullptr, 0);
    CHECK(!says("does not fit"));
    // a valid call: no GPU here, or the pageable arena refused; never a result word written before that
    st = fn(code, arena.data(), bytes, 0, offs, sizes, nums, 7, 3, res, nullptr, FEC_FLAG_ROW_PADDING);
    CHECK(st == FEC_ENODEV || (st == FEC_EINVAL && says("pageable host memory")));
    CHECK(res[0] == 0x55 && res[1] == 0x55 && res[2] == 0x55);
    fec_free(code);
}

}  // namespace

int main() {
    fec_init();
    run(fec_verify_batch_ragged, "fec_verify_batch_ragged", "mismatch");
    run(fec_locate_batch_ragged, "fec_locate_batch_ragged", "culprit");
    if (g_fail) {
        fprintf(stderr, "ragged_scrub_validate: %d check(s) failed\n", g_fail);
        return 1;
    }
    printf("ragged_scrub_validate: ok\n");
    return 0;
}
