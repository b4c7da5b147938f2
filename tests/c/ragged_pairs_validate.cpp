// ragged_pairs_validate.cpp -- the validation path of fec_locate2_batch_ragged
// and fec_correct2_batch_ragged under AddressSanitizer and
// UndefinedBehaviorSanitizer (make asan-pairs: every host object of
// libzfec_hip.so compiled with both and linked into this program).  Runs
// without a GPU: every check the header lists comes before any GPU work, so
// what is exercised is the argument checks in their order, the fit test with
// its wrap cases, the message formatting under each call's own name, and the
// end a valid call meets on a machine without a GPU (FEC_ENODEV) or with one
// (the pageable arena refused), for a shape of each path: the fused one, the
// one below the pair pass and the one cut into runs.  The arena and the
// 2 * nstripes verdict words are never written.
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
typedef int (*PairsFn)(const fec_t*, gf*, size_t, size_t, const u64*, const u64*, const unsigned*, size_t, size_t,
                       unsigned*, void*, unsigned);

int locate2(const fec_t* c, gf* a, size_t bytes, size_t bs, const u64* off, const u64* sz, const unsigned* nums,
            size_t nb, size_t ns, unsigned* out, void* stream, unsigned flags) {
    return fec_locate2_batch_ragged(c, a, bytes, bs, off, sz, nums, nb, ns, out, stream, flags);
}

// arena, offsets: what the call names its arena and its offsets in messages
void checks(PairsFn fn, const char* name, const char* arena_name, const char* offsets_name) {
    fec_t* code = fec_new(3, 10);
    CHECK(code != nullptr);
    const unsigned nums[7] = {7, 0, 4, 1, 9, 2, 5};
    const u64 sizes[3] = {8, 0, 24}, offs[3] = {0, 56, 56};
    std::vector<gf> arena(7 * 32, 0x3C);
    unsigned res[6] = {0x55, 0x55, 0x55, 0x55, 0x55, 0x55};
    const size_t bytes = arena.size();
    char want[128];
    const auto says_null = [&](const char* what) {
        snprintf(want, sizeof want, "%s: %s is NULL", name, what);
        return says(want);
    };
    const auto says_unfit = [&](int s) {
        snprintf(want, sizeof want, "%s: stripe %d does not fit %s", name, s, arena_name);
        return says(want);
    };

    CHECK(fn(nullptr, nullptr, bytes, 0, nullptr, nullptr, nullptr, 7, 3, nullptr, nullptr, 0) == FEC_EINVAL);
    CHECK(says(name) && says("invalid fec_t"));
    CHECK(fn(code, nullptr, bytes, 0, nullptr, nullptr, nullptr, 7, 3, nullptr, nullptr, 0) == FEC_EINVAL);
    CHECK(says_null(arena_name));
    CHECK(fn(code, arena.data(), bytes, 0, nullptr, nullptr, nullptr, 7, 3, nullptr, nullptr, 0) == FEC_EINVAL);
    CHECK(says_null("sizes"));
    CHECK(fn(code, arena.data(), bytes, 0, nullptr, sizes, nullptr, 7, 3, nullptr, nullptr, 0) == FEC_EINVAL);
    CHECK(says_null(offsets_name));
    CHECK(fn(code, arena.data(), bytes, 0, offs, sizes, nullptr, 7, 3, nullptr, nullptr, 0) == FEC_EINVAL);
    CHECK(says_null("block_nums"));
    CHECK(fn(code, arena.data(), bytes, 0, offs, sizes, nums, 3, 3, nullptr, nullptr, 0) == FEC_EINVAL);
    CHECK(says_null("culprit"));
    CHECK(fn(code, arena.data(), bytes, 0, offs, sizes, nums, 3, 3, res, nullptr, 0) == FEC_EINVAL);
    CHECK(says(name) && says("nothing to check"));
    const unsigned many[11] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 12};
    CHECK(fn(code, arena.data(), bytes, 0, offs, sizes, many, 11, 3, res, nullptr, 0) == FEC_EINVAL);
    CHECK(says(name) && says("only n = 10"));
    const unsigned far[4] = {5, 5, 1, 10}, twice[4] = {5, 5, 1, 9};
    CHECK(fn(code, arena.data(), bytes, 0, offs, sizes, far, 4, 3, res, nullptr, 0) == FEC_EINVAL);
    CHECK(says(name) && says("block number 10 out of range"));
    CHECK(fn(code, arena.data(), bytes, 0, offs, sizes, twice, 4, size_t(1) << 32, res, nullptr, 0) == FEC_EINVAL);
    CHECK(says(name) && says("duplicate block number 5"));
    // the stripe count, before any array is read (the arrays hold three words)
    CHECK(fn(code, arena.data(), bytes, 0, offs, sizes, nums, 7, size_t(1) << 32, res, nullptr, 0) == FEC_EINVAL);
    CHECK(says(name) && says("fewer than 2^32"));
    CHECK(fn(code, arena.data(), bytes, 0, offs, sizes, nums, 7, 0, res, nullptr, 0) == FEC_OK);
    // the fit of host-side descriptors over all nb slots, and its wrap cases
    const u64 late[3] = {0, 56, 57};
    CHECK(fn(code, arena.data(), bytes, 0, late, sizes, nums, 7, 3, res, nullptr, 0) == FEC_EINVAL);
    CHECK(says_unfit(2));
    CHECK(fn(code, arena.data(), bytes - 1, 0, offs, sizes, nums, 7, 3, res, nullptr, 0) == FEC_EINVAL);
    CHECK(says_unfit(2));
    const u64 one[1] = {16}, wrap[1] = {~0ull - 7}, zero[1] = {0};
    CHECK(fn(code, arena.data(), bytes, 0, wrap, one, nums, 7, 1, res, nullptr, 0) == FEC_EINVAL);
    CHECK(says_unfit(0));
    CHECK(fn(code, arena.data(), ~size_t(0), size_t(1) << 63, zero, one, nums, 7, 1, res, nullptr, 0) == FEC_EINVAL);
    CHECK(says_unfit(0));
    CHECK(fn(code, arena.data(), 6 * 30 + 15, 30, zero, one, nums, 7, 1, res, nullptr, 0) == FEC_EINVAL);
    CHECK(says_unfit(0));
    // a zero-size stripe is not looked at, wherever its offset points
    const u64 wild[3] = {0, 1ull << 63, 56};
    int st = fn(code, arena.data(), bytes, 0, wild, sizes, nums, 7, 3, res, nullptr, 0);
    CHECK(!says("does not fit"));
    // a valid call of each path: the fused one (c = 4), below the pair pass (c = 2), more than 8 checks (runs)
    snprintf(want, sizeof want, "%s is pageable host memory", arena_name);
    st = fn(code, arena.data(), bytes, 0, offs, sizes, nums, 7, 3, res, nullptr, FEC_FLAG_ROW_PADDING);
    CHECK(st == FEC_ENODEV || (st == FEC_EINVAL && says(name) && says(want)));
    const u64 offs5[3] = {0, 40, 40};
    st = fn(code, arena.data(), bytes, 0, offs5, sizes, nums, 5, 3, res, nullptr, 0);
    CHECK(st == FEC_ENODEV || (st == FEC_EINVAL && says(name) && says(want)));
    fec_free(code);
    // K=10/M=16 with 14 slots (c = 4): cut into runs
    code = fec_new(10, 16);
    CHECK(code != nullptr);
    unsigned wide[14];
    for (unsigned i = 0; i < 14; ++i) wide[i] = i;
    const u64 small[3] = {4, 4, 1}, woffs[3] = {0, 56, 112};
    st = fn(code, arena.data(), bytes, 0, woffs, small, wide, 14, 3, res, nullptr, 0);
    CHECK(st == FEC_ENODEV || (st == FEC_EINVAL && says(name) && says(want)));
    for (unsigned w : res) CHECK(w == 0x55);
    for (gf b : arena) CHECK(b == 0x3C);
    fec_free(code);
}

}  // namespace

int main() {
    fec_init();
    checks(locate2, "fec_locate2_batch_ragged", "src", "src_offsets");
    checks(fec_correct2_batch_ragged, "fec_correct2_batch_ragged", "blocks", "offsets");
    if (g_fail) {
        fprintf(stderr, "ragged_pairs_validate: %d check(s) failed\n", g_fail);
        return 1;
    }
    printf("ragged_pairs_validate: ok\n");
    return 0;
}
