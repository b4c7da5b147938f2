// config.cpp -- see config.hpp.
#include "config.hpp"

#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>

namespace zfec_hip {
namespace {

const char* env(const char* name) {
    const char* v = getenv(name);
    return v && *v ? v : nullptr;
}

// Default of Config::verify_fused_min.  Never below 32: launches of up to 18
// units are pinned to the two-step path by the scratch-path tests.  Measured
// (tools/verify_wide_bench.py, profiles/verify_wide_bench.json; K=10/M=16, 4 KiB
// blocks, cold): no crossover -- the fused call is ahead at every count tried,
// 16 units 0.0106 against 0.0195 ms (0.54 x), 64 units 0.0107 / 0.0196, 256
// units 0.0111 / 0.0175, 1024 units 0.0126 / 0.0223 -- so the default is the
// smallest measured count above that floor.
constexpr size_t kVerifyFusedMin = 64;

size_t env_size(const char* name, size_t dflt) {
    const char* v = env(name);
    return v ? static_cast<size_t>(strtoull(v, nullptr, 10)) : dflt;
}

Config* read_env() {
    Config* c = new Config;
    const char* w = env("ZFEC_HIP_WAIT");
    c->wait_signal = !(w && !strcmp(w, "sync"));
    c->pack_limit = env_size("ZFEC_HIP_PACK_LIMIT", size_t(4) << 20);
    c->stage_min = env_size("ZFEC_HIP_STAGE_MIN", size_t(512) << 10);
    c->zc_limit = env_size("ZFEC_HIP_ZC_LIMIT", size_t(3) << 19);  // 1.5 MiB
    const char* q = env("ZFEC_HIP_QUIET");
    c->quiet = q && q[0] == '1';
    const unsigned long long u = env_size("ZFEC_HIP_LAUNCH_UNITS", 0);
    // the kernels' own bound is < 2^32 units per launch
    c->launch_units = u >= 1024 && u < (1ull << 31) ? static_cast<size_t>(u) : size_t(1) << 31;
    c->small_lanes = env_size("ZFEC_HIP_SMALL_LANES", 2048);
    const size_t sc = env_size("ZFEC_HIP_STAGE_CHUNK", 0);
    c->stage_chunk = sc >= (64u << 10) ? sc / 4096 * 4096 : 0;
    // the launch path ignores a value past its own cap (CUs x 8192, known there)
    c->grid_cap = env_size("ZFEC_HIP_GRID_CAP", 0);
    const size_t vs = env_size("ZFEC_HIP_VERIFY_SCRATCH", 0), vmax = size_t(64) << 20;
    // (255 check rows of at least 128 bytes each must fit)
    c->verify_scratch = vs >= (64u << 10) && vs < vmax ? vs : vmax;
    // 2-KiB units (ceil(sz / 2048) x nstripes) from which fec_verify_batch's wide
    // shapes take the fused kernel; 0 is read as 1, 4294967295 turns it off.
    const size_t vf = env_size("ZFEC_HIP_VERIFY_FUSED_MIN", kVerifyFusedMin);
    c->verify_fused_min = vf ? vf : 1;
    const char* mf = env("ZFEC_HIP_MIXED_FUSED");
    c->mixed_fused = !(mf && mf[0] == '0');
    return c;
}

std::atomic<const Config*> g_cfg{nullptr};
std::mutex g_mu;

}  // namespace

const Config& config() {
    const Config* c = g_cfg.load(std::memory_order_acquire);
    if (c) return *c;
    std::lock_guard<std::mutex> g(g_mu);
    c = g_cfg.load(std::memory_order_relaxed);
    if (!c) {
        c = read_env();
        g_cfg.store(c, std::memory_order_release);
    }
    return *c;
}

void reload_config() {
    std::lock_guard<std::mutex> g(g_mu);
    g_cfg.store(read_env(), std::memory_order_release);  // the old object is kept: readers may hold it
}

}  // namespace zfec_hip
