// fec_abi.cpp -- the C-ABI of libzfec_hip.so (include/zfec_hip.h).
//
// Part 1 replaces /root/reference/zfec/fec.h:33-57 (fec_init, fec_new,
// fec_free, fec_encode, fec_decode) and the two helpers fec.c also exports.
// Host-side work here is O(k^3) matrix algebra and argument checking; every
// output byte is produced by the HIP kernels in kernels.hip.  Host buffers are
// staged through per-thread device buffers; device buffers are used in place.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <memory>
#include <new>
#include <optional>
#include <stdexcept>
#include <string>
#include <sys/mman.h>
#include <thread>
#include <unistd.h>

#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/zfec_hip.h"
#include "bitslice.hpp"
#include "config.hpp"
#include "gf256.hpp"
#include "host_pool.hpp"
#include "kernels.hpp"

#define FEC_API extern "C" __attribute__((visibility("default")))

namespace zfec_hip {
namespace {

constexpr unsigned long kFecMagic = 0xFECC0DECUL;  // zfec/fec.c:421

thread_local int t_status = FEC_OK;
thread_local char t_msg[256] = "";

int set_status(int st, const char* fmt = nullptr, ...) {
    t_status = st;
    if (fmt) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(t_msg, sizeof t_msg, fmt, ap);
        va_end(ap);
    } else {
        t_msg[0] = '\0';
    }
    return st;
}

int hip_fail(hipError_t e, const char* what) {
    return set_status(FEC_EHIP, "%s: %s", what, hipGetErrorString(e));
}

// No C++ exception crosses the C-ABI: a failed allocation (or a thread the
// system cannot create) inside a call becomes its status.
template <class F>
int guarded(F&& f) {
    try {
        return f();
    } catch (const std::bad_alloc&) {
        return set_status(FEC_ENOMEM, "out of host memory");
    } catch (const std::exception& x) {
        return set_status(FEC_ENOMEM, "host resources exhausted: %s", x.what());
    }
}

unsigned long magic_of(const fec_t* p) {
    return ((kFecMagic ^ p->k) ^ p->n) ^ reinterpret_cast<unsigned long>(p->enc_matrix);
}

bool valid_code(const fec_t* c) { return c && c->enc_matrix && c->magic == magic_of(c); }

// ---- per-thread, per-device staging -----------------------------------------

constexpr int kStageSlots = 3;  // staged host path: copy-in | kernel | copy-out

struct DevCtx {
    hipStream_t stream = nullptr;  // library stream: kernels of the host path, sync calls
    void* dbuf = nullptr;
    size_t dcap = 0;
    void* hbuf = nullptr;  // pinned
    void* hbuf_dev = nullptr;  // its address in the device's view (kernels read / write it over PCIe)
    size_t hcap = 0;
    void* sbuf = nullptr;  // pinned staging slots of the staged host path
    void* sbuf_dev = nullptr;
    size_t scap = 0;
    hipEvent_t ev_stg[kStageSlots] = {};
    uint32_t* flag = nullptr;      // pinned completion word of small synchronous calls
    uint32_t* flag_dev = nullptr;  // its address in the device's view
    uint32_t seq = 0;
    // fec_verify_batch: the expected check rows of the two-step path, and the
    // mismatch words of a call whose `mismatch` is host memory.  Calls of this
    // thread on different streams share them: each use waits (on the GPU) for
    // the event recorded after the previous one.
    void* vbuf = nullptr;
    size_t vcap = 0;
    void* vmask = nullptr;
    size_t vmask_cap = 0;
    hipEvent_t ev_verify = nullptr;
    bool verify_busy = false;
};

struct ThreadCtx {
    std::unordered_map<int, DevCtx> dev;
    ~ThreadCtx() {
        for (auto& kv : dev) {
            int cur = 0;
            if (hipGetDevice(&cur) != hipSuccess) continue;
            if (hipSetDevice(kv.first) != hipSuccess) continue;
            DevCtx& d = kv.second;
            if (d.stream) (void)hipStreamDestroy(d.stream);
            for (int i = 0; i < kStageSlots; ++i)
                if (d.ev_stg[i]) (void)hipEventDestroy(d.ev_stg[i]);
            if (d.dbuf) (void)hipFree(d.dbuf);
            if (d.hbuf) (void)hipHostFree(d.hbuf);
            if (d.sbuf) (void)hipHostFree(d.sbuf);
            if (d.flag) (void)hipHostFree(d.flag);
            if (d.ev_verify) (void)hipEventSynchronize(d.ev_verify), (void)hipEventDestroy(d.ev_verify);
            if (d.vbuf) (void)hipFree(d.vbuf);
            if (d.vmask) (void)hipFree(d.vmask);
            (void)hipSetDevice(cur);
        }
    }
};

thread_local ThreadCtx t_ctx;

int dev_ctx(int device, DevCtx** out) {
    DevCtx& d = t_ctx.dev[device];
    if (!d.stream) {
        hipError_t e = hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking);
        if (e != hipSuccess) return hip_fail(e, "hipStreamCreateWithFlags");
    }
    *out = &d;
    return FEC_OK;
}

int ensure_dbuf(DevCtx& d, size_t bytes) {
    if (bytes <= d.dcap) return FEC_OK;
    if (d.dbuf) {
        (void)hipStreamSynchronize(d.stream);
        (void)hipFree(d.dbuf);
        d.dbuf = nullptr;
        d.dcap = 0;
    }
    const size_t cap = std::max<size_t>(bytes, 1u << 20);
    hipError_t e = hipMalloc(&d.dbuf, cap);
    if (e != hipSuccess) return set_status(FEC_ENOMEM, "hipMalloc(%zu): %s", cap, hipGetErrorString(e));
    d.dcap = cap;
    return FEC_OK;
}

int ensure_hbuf(DevCtx& d, size_t bytes) {
    if (bytes <= d.hcap) return FEC_OK;
    if (d.hbuf) {
        (void)hipStreamSynchronize(d.stream);
        (void)hipHostFree(d.hbuf);
        d.hbuf = nullptr;
        d.hbuf_dev = nullptr;
        d.hcap = 0;
    }
    const size_t cap = std::max<size_t>(bytes, 1u << 20);
    hipError_t e = hipHostMalloc(&d.hbuf, cap, hipHostMallocDefault);
    if (e != hipSuccess) return set_status(FEC_ENOMEM, "hipHostMalloc(%zu): %s", cap, hipGetErrorString(e));
    if ((e = hipHostGetDevicePointer(&d.hbuf_dev, d.hbuf, 0)) != hipSuccess || !d.hbuf_dev) {
        (void)hipGetLastError();
        d.hbuf_dev = d.hbuf;  // unified addressing: the host address is valid on the device
    }
    d.hcap = cap;
    return FEC_OK;
}

// Device holding p, or -1 for host memory.  For page-locked host memory
// (hipHostMalloc / hipHostRegister, torch pin_memory) *pinned is set and
// *dev_ptr is the address a kernel uses to read / write it over PCIe.
int pointer_device(const void* p, bool* pinned = nullptr, void** dev_ptr = nullptr) {
    hipPointerAttribute_t a;
    if (pinned) *pinned = false;
    if (dev_ptr) *dev_ptr = nullptr;
    hipError_t e = hipPointerGetAttributes(&a, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    if (a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged) return a.device;
    if (a.type == hipMemoryTypeHost) {
        if (pinned) *pinned = true;
        if (dev_ptr) *dev_ptr = a.devicePointer ? a.devicePointer : const_cast<void*>(p);
    }
    return -1;
}

int gpu_available() {
    // the device count of a process does not change: cached once positive
    static std::atomic<int> cached{0};
    const int c = cached.load(std::memory_order_relaxed);
    if (c > 0) return c;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    if (n > 0) cached.store(n, std::memory_order_relaxed);
    return n;
}

// Small synchronous calls (one-workgroup register-kernel launches): the
// kernel publishes completion in pinned host memory and the calling thread
// spins on it -- launch to return 6.4-6.9 us against 12.2 us through
// hipStreamSynchronize (tools/mb_sync.hip, profiles/r02_sync_probe.log).
// The stream is queried every 1024 spins, so an error ends the wait; past
// 200 us it blocks in hipStreamSynchronize.  ZFEC_HIP_WAIT=sync turns it off.
uint32_t* signal_slot(DevCtx& d) {
    if (!config().wait_signal) return nullptr;
    if (!d.flag) {
        void* p = nullptr;
        if (hipHostMalloc(&p, 64, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        void* pd = nullptr;
        if (hipHostGetDevicePointer(&pd, p, 0) != hipSuccess || !pd) {
            (void)hipGetLastError();
            pd = p;
        }
        d.flag = static_cast<uint32_t*>(p);
        d.flag_dev = static_cast<uint32_t*>(pd);
        __atomic_store_n(d.flag, 0u, __ATOMIC_RELEASE);
    }
    if (++d.seq == 0) d.seq = 1;
    return d.flag_dev;
}

hipError_t wait_signal(DevCtx& d, hipStream_t st) {
    const uint32_t seq = d.seq;
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t n = 1;; ++n) {
        if (__atomic_load_n(d.flag, __ATOMIC_ACQUIRE) == seq) return hipSuccess;
        if ((n & 1023u) == 0) {
            const hipError_t q = hipStreamQuery(st);
            if (q == hipSuccess) return hipSuccess;  // the stream is idle: the kernel has finished
            if (q != hipErrorNotReady) return q;
            if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(200)) break;
        }
    }
    return hipStreamSynchronize(st);
}

// RAII: restore the caller's current device.
struct DeviceGuard {
    int prev = -1;
    bool changed = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) {
            (void)hipSetDevice(dev);
            changed = true;
        }
    }
    ~DeviceGuard() {
        if (changed && prev >= 0) (void)hipSetDevice(prev);
    }
};

// ---- the engine: apply an r x k matrix to k blocks -----------------------------

constexpr size_t align_up_4k(size_t x) { return (x + 4095) / 4096 * 4096; }

// in[j] / out[i] are device pointers (block bases of stripe 0); stripes are
// in_sstride / out_sstride apart; coef is r x k with rows coef_stride apart.
// Splits into launches that respect the kernels' limits: <= kMaxOut outputs
// per launch; all k inputs in one pass where a bit-sliced kernel takes them
// (wide_launch_ok), otherwise groups of <= kMaxIn inputs, later groups
// XOR-accumulating, and <= kMaxCoef coefficients per launch; at most
// Config::launch_units kMinChunk-byte units per launch.  Blocks longer than
// that are cut into byte ranges of their own launches: output byte x depends
// only on byte x of the inputs (zfec/fec.c:494-503, :547-556).
thread_local unsigned t_launches = 0;  // launches made by this thread (the signal path checks it made one)
thread_local int t_last_wait = 0;      // 1: the last synchronous small call waited on its kernel's signal (fec_last_wait)

int apply_matrix_range(const uint8_t* coef, unsigned coef_stride, unsigned k, unsigned r, const uint8_t* const* in,
                       uint8_t* const* out, size_t sz, size_t nstripes, size_t in_sstride, size_t out_sstride,
                       hipStream_t stream);

int apply_matrix(const uint8_t* coef /* r x k */, unsigned k, unsigned r, const uint8_t* const* in,
                 uint8_t* const* out, size_t sz, size_t nstripes, size_t in_sstride, size_t out_sstride,
                 hipStream_t stream, unsigned coef_stride = 0) {
    if (r == 0 || sz == 0 || nstripes == 0) return FEC_OK;
    if (!coef_stride) coef_stride = k;
    const size_t cps = (sz + kMinChunk - 1) / kMinChunk;
    const size_t max_units = config().launch_units;
    if (cps <= max_units)
        return apply_matrix_range(coef, coef_stride, k, r, in, out, sz, nstripes, in_sstride, out_sstride, stream);
    // near-equal byte ranges on 4 KiB boundaries, each within the unit limit
    const size_t pieces = (cps + max_units - 1) / max_units;
    const size_t piece = align_up_4k((sz + pieces - 1) / pieces);
    const uint8_t* pin[kMaxWideIn];
    uint8_t* pout[kMaxWideIn];
    for (size_t b0 = 0; b0 < sz; b0 += piece) {
        const size_t len = std::min(piece, sz - b0);
        for (unsigned j = 0; j < k; ++j) pin[j] = in[j] + b0;
        for (unsigned i = 0; i < r; ++i) pout[i] = out[i] + b0;
        if (apply_matrix_range(coef, coef_stride, k, r, pin, pout, len, nstripes, in_sstride, out_sstride, stream))
            return t_status;
    }
    return FEC_OK;
}

int apply_matrix_range(const uint8_t* coef, unsigned coef_stride, unsigned k, unsigned r, const uint8_t* const* in,
                       uint8_t* const* out, size_t sz, size_t nstripes, size_t in_sstride, size_t out_sstride,
                       hipStream_t stream) {
    const size_t cps = (sz + kMinChunk - 1) / kMinChunk;
    const size_t stripes_per_launch = std::max<size_t>(1, config().launch_units / cps);
    // wide codes: every input in one bit-sliced pass per row group
    // (not under graph capture: the one-pass wide kernels read device-side
    // tables filled at enqueue time; the passes' kernels take their arguments)
    const bool wide = k > static_cast<unsigned>(kMaxIn) &&
                      wide_launch_ok(k, r, sz, std::min(stripes_per_launch, nstripes)) && !stream_capturing(stream);
    const unsigned kstep = wide ? k : static_cast<unsigned>(kMaxIn);
    const uint8_t* pin[kMaxWideIn];
    uint8_t* pout[kMaxWideIn];
    for (unsigned j0 = 0; j0 < k; j0 += kstep) {
        const unsigned kg = std::min<unsigned>(kstep, k - j0);
        // wide: every row in one launch (matapply_bsg walks row groups itself,
        // the JIT takes k * r <= kJitMaxCoef)
        const unsigned rmax = wide ? r : std::max<unsigned>(1, std::min<unsigned>(kMaxOut, kMaxCoef / kg));
        const unsigned ngroups = (r + rmax - 1) / rmax;
        for (unsigned g = 0; g < ngroups; ++g) {
            // near-equal row groups
            const unsigned i0 = g * r / ngroups, rg = (g + 1) * r / ngroups - i0;
            for (size_t s0 = 0; s0 < nstripes; s0 += stripes_per_launch) {
                const size_t ns = std::min(stripes_per_launch, nstripes - s0);
                for (unsigned j = 0; j < kg; ++j) pin[j] = in[j0 + j] + s0 * in_sstride;
                for (unsigned i = 0; i < rg; ++i) pout[i] = out[i0 + i] + s0 * out_sstride;
                ApplySpec a;
                a.coef = coef + size_t(i0) * coef_stride + j0;
                a.coef_stride = coef_stride;
                a.k = kg;
                a.r = rg;
                a.in = pin;
                a.out = pout;
                a.sz = sz;
                a.nstripes = ns;
                a.in_sstride = in_sstride;
                a.out_sstride = out_sstride;
                a.accumulate = j0 > 0;
                ++t_launches;
                const hipError_t e = launch_apply(a, stream);
                if (e != hipSuccess) return hip_fail(e, "launch_apply");
            }
        }
    }
    return FEC_OK;
}

// ---- host/device pointer marshalling for the fec.h-shaped entry points -------

struct Marshal {
    int device = -1;
    std::vector<const uint8_t*> din;
    std::vector<uint8_t*> dout;
    std::vector<int> in_host, out_host;  // indices of host-memory blocks
    bool all_pinned = true;              // every host block is page-locked
    std::vector<const uint8_t*> zin;     // kernel-visible address of every block (zero-copy), when all_pinned
    std::vector<uint8_t*> zout;
};

// Classify pointers and pick the device.  All device pointers must live on one device.
int classify(const gf* const* in, size_t nin, gf* const* out, size_t nout, Marshal& m) {
    m.in_host.clear();
    m.out_host.clear();
    m.all_pinned = true;
    m.zin.assign(in, in + nin);
    m.zout.assign(out, out + nout);
    int dev = -1;
    auto visit = [&](const void* p, bool is_in, size_t idx) -> int {
        if (!p) return set_status(FEC_EINVAL, "%s block %zu is NULL", is_in ? "input" : "output", idx);
        bool pinned = false;
        void* dp = nullptr;
        const int d = pointer_device(p, &pinned, &dp);
        if (d < 0) {
            (is_in ? m.in_host : m.out_host).push_back(static_cast<int>(idx));
            m.all_pinned = m.all_pinned && pinned;
            if (pinned) {
                if (is_in)
                    m.zin[idx] = static_cast<const uint8_t*>(dp);
                else
                    m.zout[idx] = static_cast<uint8_t*>(dp);
            }
        } else if (dev < 0) {
            dev = d;
        } else if (d != dev) {
            return set_status(FEC_EINVAL, "blocks live on different devices (%d, %d)", dev, d);
        }
        return FEC_OK;
    };
    for (size_t i = 0; i < nin; ++i)
        if (visit(in[i], true, i)) return t_status;
    for (size_t i = 0; i < nout; ++i)
        if (visit(out[i], false, i)) return t_status;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return set_status(FEC_ENODEV, "no current HIP device");
    m.device = dev;
    return FEC_OK;
}

// Host blocks of up to Config::pack_limit bytes in total (4 MiB) go through
// one pinned bounce buffer (one H2D / D2H each way); larger ones take the
// staged path.  From Config::stage_min bytes (512 KiB), blocks of at least
// kStageMinBlock bytes take the staged path too: its overlapped copy-in / kernel / copy-out beats the bounce
// buffer's serial memcpy / DMA / kernel / DMA / memcpy (K=3/M=10 from bytes,
// 1 MiB stripe: 137 vs 209 us per encode; 256 KiB stripe: 69 vs 77 us), but
// not for many small blocks (K=20/M=60, 256 KiB stripe of 13 KB blocks: 260
// vs 122 us; tools/archive/host_lat_ab.py, profiles/r02_host_lat_ab.log).
constexpr size_t kStageMinBlock = size_t(64) << 10;
// Up to Config::zc_limit bytes (1.5 MiB; calls of k <= 4, r <= 8 up to that
// size stay on the bounce buffer, run_single) the kernel accesses the bounce
// buffer in place.  Round 2 stopped at 256 KiB; an interleaved A/B of 100-150
// KB K=3/M=10 stripes from bytes (tools/archive/small_ab_inproc.py --set zc,
// profiles/r03_zc_ab.log): encode 44.5-51.3 -> 25.1-33.0 us, decode
// 17.0-38.3 -> 16.9-19.8 us against one H2D and one D2H copy.

constexpr size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Kernel-visible address of the host block [p, p + n), or nullptr unless the
// whole block is page-locked (first and last byte mapped at the same offset).
const uint8_t* mapped_block(const void* p, size_t n) {
    bool pa = false, pb = false;
    void *da = nullptr, *db = nullptr;
    const char* last = static_cast<const char*>(p) + (n ? n - 1 : 0);
    if (pointer_device(p, &pa, &da) >= 0 || !pa) return nullptr;
    if (pointer_device(last, &pb, &db) >= 0 || !pb) return nullptr;
    if (static_cast<char*>(db) - static_cast<char*>(da) != last - static_cast<const char*>(p)) return nullptr;
    return static_cast<const uint8_t*>(da);
}

// ---- the memory and stream of a batched call ------------------------------------------
// One block buffer of a batched call: [p, p + extent), `label` in messages.
struct BatchBuf {
    const gf* p;
    size_t extent;
    const char* label;
};

// What resolve_batch yields: the kernel-visible address of each buffer (device
// memory as it is, page-locked host memory as the device maps it), the device
// -- current while `guard` lives -- its per-thread context and the stream.
struct BatchMem {
    const gf* z[3] = {nullptr, nullptr, nullptr};
    int bdev[3] = {-1, -1, -1};  // each buffer's device, -1: host memory
    int dev = -1;
    DevCtx* d = nullptr;
    hipStream_t st = nullptr;
    std::optional<DeviceGuard> guard;
};

// Resolves the buffers (at most three) of the call `fn`: one pointer query per
// buffer, a second pair for a page-locked one.  Pageable host memory is
// refused -- except with fn == nullptr (fec_encode_batch / fec_decode_batch,
// which stage it): its z stays null.  `side` (may be null) names a further
// pointer the caller found on device side_dev (-1: host memory), which must
// not be another device than the blocks'.  no_capture (may be null): why the
// call cannot be captured into a graph.
int resolve_batch(BatchMem& m, const char* fn, const BatchBuf* bufs, int nbufs, const char* side, int side_dev,
                  void* stream, unsigned flags, const char* no_capture) {
    for (int i = 0; i < nbufs; ++i) m.bdev[i] = pointer_device(bufs[i].p);
    for (int i = 0; i < nbufs; ++i) {
        m.z[i] = m.bdev[i] >= 0 ? bufs[i].p : mapped_block(bufs[i].p, bufs[i].extent);
        if (!m.z[i] && fn)
            return set_status(FEC_EINVAL, "%s takes device or page-locked host memory: %s is pageable host memory, "
                                          "which this call does not stage", fn, bufs[i].label);
    }
    for (int i = 0; i < nbufs; ++i) {
        if (m.bdev[i] < 0) continue;
        if (m.dev >= 0 && m.dev != m.bdev[i])
            return set_status(FEC_EINVAL, "batched entry points take memory on one device");
        m.dev = m.bdev[i];
    }
    if (m.dev >= 0 && side_dev >= 0 && side_dev != m.dev)
        return set_status(FEC_EINVAL, "%s lives on device %d, the blocks on device %d", side, side_dev, m.dev);
    if (m.dev < 0) m.dev = side_dev;
    if (m.dev < 0 && hipGetDevice(&m.dev) != hipSuccess) return set_status(FEC_ENODEV, "no current HIP device");
    m.guard.emplace(m.dev);
    if (dev_ctx(m.dev, &m.d)) return t_status;
    m.st = (flags & FEC_FLAG_LIBRARY_STREAM) ? m.d->stream : static_cast<hipStream_t>(stream);
    if (no_capture && stream_capturing(m.st))
        return set_status(FEC_EINVAL, "%s: the stream is being captured into a graph (%s)", fn, no_capture);
    return FEC_OK;
}

constexpr char kCaptureTables[] = "the pattern tables are uploaded when the call is made";
constexpr char kCaptureMemory[] = "the call uses memory the library owns and reuses";

// Bytes of every host block per staged chunk: ZFEC_HIP_STAGE_CHUNK, else
// at most a quarter of the block (so that copy-in, kernel and copy-out of
// consecutive chunks overlap) and at most about 16 MiB of staging per chunk
// over all host blocks, in whole 64 KiB
// (K=3/M=10, 64 MiB from bytes: 8 MiB chunks 8.7 GB/s encode, 16-20 MiB 9.3;
// 2.5 MiB 6.4; profiles/r02_host_stage_ab.log).
size_t staged_chunk(size_t nblocks, size_t sz) {
    if (const size_t v = config().stage_chunk) return v;
    const size_t total = size_t(16) << 20, g = size_t(64) << 10;
    const size_t by_total = total / std::max<size_t>(1, nblocks) / g * g;
    const size_t quarter = (sz + 4 * g - 1) / (4 * g) * g;  // at least 4 chunks, so the stages overlap
    return std::max<size_t>(256u << 10, std::min(by_total, quarter));
}

int ensure_sbuf(DevCtx& d, size_t bytes) {
    if (!d.ev_stg[0])
        for (int i = 0; i < kStageSlots; ++i) {
            hipError_t e = hipEventCreateWithFlags(&d.ev_stg[i], hipEventDisableTiming);
            if (e != hipSuccess) return hip_fail(e, "staging events");
        }
    if (bytes <= d.scap) return FEC_OK;
    if (d.sbuf) {
        (void)hipDeviceSynchronize();  // no kernel of an earlier call may still use the old slots
        (void)hipHostFree(d.sbuf);
        d.sbuf = d.sbuf_dev = nullptr;
        d.scap = 0;
    }
    hipError_t e = hipHostMalloc(&d.sbuf, bytes, hipHostMallocDefault);
    if (e != hipSuccess) return set_status(FEC_ENOMEM, "hipHostMalloc(%zu): %s", bytes, hipGetErrorString(e));
    if ((e = hipHostGetDevicePointer(&d.sbuf_dev, d.sbuf, 0)) != hipSuccess || !d.sbuf_dev) {
        (void)hipGetLastError();
        d.sbuf_dev = d.sbuf;
    }
    d.scap = bytes;
    return FEC_OK;
}

// Large pageable host blocks, staged: nothing of the caller's is page-locked.
// The byte range is cut into chunks; for chunk c the host threads (HostPool)
// copy the input blocks' bytes into a pinned staging slot, the kernel reads
// that slot and writes the outputs into the slot over PCIe (zero-copy), and
// the threads copy the outputs out into the caller's blocks -- faulting in
// fresh output pages (new `bytes` objects, zfec/_fecmodule.c:206-242) on every
// pool thread at once.  kStageSlots slots rotate, so copy-in of chunk c + 1 and
// copy-out of chunk c - 1 run while chunk c's kernel does.  Replaces
// hipHostRegister of every block (run_pageable), whose cost is the kernel
// mapping each fresh page one by one.  Device-resident and
// caller-locked blocks are read / written in place.
int run_staged(DevCtx& d, const uint8_t* coef, unsigned k, unsigned r, const gf* const* in, gf* const* out,
               size_t sz, Marshal& m, hipStream_t st) {
    std::vector<char> host_in(k, 0), host_out(r, 0);
    std::vector<const uint8_t*> base_in(m.zin);  // kernel-visible bases of device / caller-locked blocks
    std::vector<uint8_t*> base_out(m.zout);
    std::vector<unsigned> sin, sout;  // staged blocks
    for (int i : m.in_host) {
        const uint8_t* z = mapped_block(in[i], sz);
        if (z) base_in[i] = z;
        else {
            host_in[i] = 1;
            sin.push_back(static_cast<unsigned>(i));
        }
    }
    for (int i : m.out_host) {
        const uint8_t* z = mapped_block(out[i], sz);
        if (z) base_out[i] = const_cast<uint8_t*>(z);
        else {
            host_out[i] = 1;
            sout.push_back(static_cast<unsigned>(i));
        }
    }
    const size_t nin = sin.size(), nout = sout.size();
    const size_t C = staged_chunk(nin + nout, sz);
    const size_t slot_bytes = C * (nin + nout);
    if (ensure_sbuf(d, slot_bytes * kStageSlots)) return t_status;
    uint8_t* const hs = static_cast<uint8_t*>(d.sbuf);
    uint8_t* const ds = static_cast<uint8_t*>(d.sbuf_dev);
    HostPool& pool = HostPool::get();
    CopyLatch lin[kStageSlots], lout[kStageSlots];
    const size_t nchunks = (sz + C - 1) / C;

    auto stage_in = [&](size_t c) {
        const int s = static_cast<int>(c % kStageSlots);
        const size_t off = c * C, len = std::min(C, sz - off);
        for (size_t q = 0; q < nin; ++q)
            pool.copy_async(hs + s * slot_bytes + q * C, in[sin[q]] + off, len, &lin[s], len);
    };
    auto copy_out = [&](size_t c) {
        const int s = static_cast<int>(c % kStageSlots);
        const size_t off = c * C, len = std::min(C, sz - off);
        const size_t piece = std::max<size_t>(256u << 10, len / 4);
        for (size_t q = 0; q < nout; ++q)
            pool.copy_async(out[sout[q]] + off, hs + s * slot_bytes + (nin + q) * C, len, &lout[s], piece);
    };
    // every queued copy references the caller's buffers and the slots: all of
    // them finish before this returns, whatever the outcome
    auto drain = [&](int status) {
        (void)hipStreamSynchronize(st);
        for (int s = 0; s < kStageSlots; ++s) {
            pool.wait(&lin[s]);
            pool.wait(&lout[s]);
        }
        return status;
    };
    std::vector<const uint8_t*> zin(k);
    std::vector<uint8_t*> zout(r);
    hipError_t e;
    try {  // a failed allocation while queueing copies: drain what was queued
    stage_in(0);
    for (size_t c = 0; c < nchunks; ++c) {
        const int s = static_cast<int>(c % kStageSlots);
        const size_t off = c * C, len = std::min(C, sz - off);
        pool.wait(&lin[s]);  // this chunk's inputs are in the slot
        pool.wait(&lout[s]);  // the slot's previous outputs have been copied out
        for (unsigned j = 0; j < k; ++j) zin[j] = base_in[j] + off;
        for (unsigned i = 0; i < r; ++i) zout[i] = base_out[i] + off;
        for (size_t q = 0; q < nin; ++q) zin[sin[q]] = ds + s * slot_bytes + q * C;
        for (size_t q = 0; q < nout; ++q) zout[sout[q]] = ds + s * slot_bytes + (nin + q) * C;
        if (apply_matrix(coef, k, r, zin.data(), zout.data(), len, 1, 0, 0, st)) return drain(t_status);
        if ((e = hipEventRecord(d.ev_stg[s], st)) != hipSuccess) return drain(hip_fail(e, "hipEventRecord"));
        if (c + 1 < nchunks) {
            // the next slot's inputs were last read by chunk c + 1 - kStageSlots,
            // synchronised below in an earlier iteration (kStageSlots >= 2)
            stage_in(c + 1);
        }
        if (c >= 1) {
            const int sp = static_cast<int>((c - 1) % kStageSlots);
            e = hipEventSynchronize(d.ev_stg[sp]);
            if (e != hipSuccess)
                return drain(hip_fail(e, "hipEventSynchronize"));
            copy_out(c - 1);
        }
    }
    if ((e = hipEventSynchronize(d.ev_stg[(nchunks - 1) % kStageSlots])) != hipSuccess)
        return drain(hip_fail(e, "hipEventSynchronize"));
    copy_out(nchunks - 1);
    } catch (const std::exception& x) {
        return drain(set_status(FEC_ENOMEM, "staged host path: %s", x.what()));
    }
    drain(FEC_OK);
    return set_status(FEC_OK);
}

// Batched calls on pageable host memory (fec_encode_batch / fec_decode_batch
// with a src or dst the GPU cannot address), staged like run_staged but cut
// into groups of whole stripes: the host pool copies a group's input rows
// into a pinned slot, one batched launch runs the group on the slot, and the
// pool copies the output rows out -- only the rows, so bytes between rows
// and past sz in the caller's arrays are never written.  In the slot a
// group's rows are packed [stripe][block][sz], or [block][stripe][sz] when the
// caller's side is block-major (stripe stride == sz), which keeps the
// block-major launch shape.  A side in device or page-locked memory is used
// in place (`src` / `dst` are then kernel-visible addresses).
int run_batch_staged(DevCtx& d, const uint8_t* coef, unsigned k, unsigned r, const gf* src, size_t sbs, size_t sss,
                     bool src_host, gf* dst, size_t dbs, size_t dss, bool dst_host, size_t sz, size_t ns,
                     hipStream_t st) {
    const bool in_bm = sss == sz, out_bm = dss == sz;
    const size_t per = (src_host ? size_t(k) * sz : 0) + (dst_host ? size_t(r) * sz : 0);
    size_t gs = std::max<size_t>(1, (size_t(16) << 20) / std::max<size_t>(1, per));
    if (ns >= 4) gs = std::min(gs, (ns + 3) / 4);  // at least 4 groups, so the stages overlap
    gs = std::min(gs, ns);
    const size_t in_bytes = align_up(src_host ? gs * k * sz : 0, 256);
    const size_t out_bytes = align_up(dst_host ? gs * r * sz : 0, 256);
    const size_t slot_bytes = in_bytes + out_bytes;
    if (ensure_sbuf(d, slot_bytes * kStageSlots)) return t_status;
    uint8_t* const hs = static_cast<uint8_t*>(d.sbuf);
    uint8_t* const ds = static_cast<uint8_t*>(d.sbuf_dev);
    HostPool& pool = HostPool::get();
    CopyLatch lin[kStageSlots], lout[kStageSlots];
    const size_t ngroups = (ns + gs - 1) / gs;
    // stripes per copy task when rows are copied one stripe at a time
    const size_t task_stripes = std::max<size_t>(1, (size_t(1) << 20) / std::max<size_t>(1, per));

    // rows of stripes [s0, s0 + n) between the caller's array (block stride
    // bs, stripe stride ss) and a slot; `to_slot` picks the direction
    auto move_rows = [&](uint8_t* slot, gf* user, size_t bs, size_t ss, unsigned nb, bool bm, size_t s0, size_t n,
                         bool to_slot, CopyLatch* latch) {
        if (bm) {  // block b of the group: n*sz contiguous bytes on both sides
            for (unsigned b = 0; b < nb; ++b) {
                uint8_t* sp = slot + size_t(b) * n * sz;
                uint8_t* up = user + b * bs + s0 * sz;
                if (to_slot)
                    pool.copy_async(sp, up, n * sz, latch);
                else
                    pool.copy_async(up, sp, n * sz, latch);
            }
            return;
        }
        for (size_t t0 = 0; t0 < n; t0 += task_stripes) {
            const size_t t1 = std::min(n, t0 + task_stripes);
            pool.run_async(
                [=]() {
                    for (size_t s = t0; s < t1; ++s) {
                        uint8_t* sp = slot + s * nb * sz;
                        uint8_t* up = user + (s0 + s) * ss;
                        if (bs == sz) {  // the stripe's rows are contiguous
                            if (to_slot)
                                std::memcpy(sp, up, nb * sz);
                            else
                                std::memcpy(up, sp, nb * sz);
                            continue;
                        }
                        for (unsigned b = 0; b < nb; ++b) {
                            if (to_slot)
                                std::memcpy(sp + b * sz, up + b * bs, sz);
                            else
                                std::memcpy(up + b * bs, sp + b * sz, sz);
                        }
                    }
                },
                latch);
        }
    };
    auto group = [&](size_t g, size_t* s0, size_t* n) {
        *s0 = g * gs;
        *n = std::min(gs, ns - *s0);
    };
    auto stage_in = [&](size_t g) {
        if (!src_host) return;
        size_t s0, n;
        group(g, &s0, &n);
        const int s = static_cast<int>(g % kStageSlots);
        move_rows(hs + s * slot_bytes, const_cast<gf*>(src), sbs, sss, k, in_bm, s0, n, true, &lin[s]);
    };
    auto copy_out = [&](size_t g) {
        if (!dst_host) return;
        size_t s0, n;
        group(g, &s0, &n);
        const int s = static_cast<int>(g % kStageSlots);
        move_rows(hs + s * slot_bytes + in_bytes, dst, dbs, dss, r, out_bm, s0, n, false, &lout[s]);
    };
    auto drain = [&](int status) {
        (void)hipStreamSynchronize(st);
        for (int s = 0; s < kStageSlots; ++s) {
            pool.wait(&lin[s]);
            pool.wait(&lout[s]);
        }
        return status;
    };
    std::vector<const uint8_t*> zin(k);
    std::vector<uint8_t*> zout(r);
    hipError_t e;
    try {  // a failed allocation while queueing copies: drain what was queued
    stage_in(0);
    for (size_t g = 0; g < ngroups; ++g) {
        const int s = static_cast<int>(g % kStageSlots);
        size_t s0, n;
        group(g, &s0, &n);
        pool.wait(&lin[s]);
        pool.wait(&lout[s]);
        size_t iss = sss, oss = dss;
        for (unsigned j = 0; j < k; ++j) zin[j] = src + j * sbs + s0 * sss;
        for (unsigned i = 0; i < r; ++i) zout[i] = dst + i * dbs + s0 * dss;
        if (src_host) {
            uint8_t* b = ds + s * slot_bytes;
            for (unsigned j = 0; j < k; ++j) zin[j] = b + (in_bm ? size_t(j) * n * sz : size_t(j) * sz);
            iss = in_bm ? sz : size_t(k) * sz;
        }
        if (dst_host) {
            uint8_t* b = ds + s * slot_bytes + in_bytes;
            for (unsigned i = 0; i < r; ++i) zout[i] = b + (out_bm ? size_t(i) * n * sz : size_t(i) * sz);
            oss = out_bm ? sz : size_t(r) * sz;
        }
        if (apply_matrix(coef, k, r, zin.data(), zout.data(), sz, n, iss, oss, st)) return drain(t_status);
        if ((e = hipEventRecord(d.ev_stg[s], st)) != hipSuccess) return drain(hip_fail(e, "hipEventRecord"));
        if (g + 1 < ngroups) stage_in(g + 1);
        if (g >= 1) {
            if ((e = hipEventSynchronize(d.ev_stg[(g - 1) % kStageSlots])) != hipSuccess)
                return drain(hip_fail(e, "hipEventSynchronize"));
            copy_out(g - 1);
        }
    }
    if ((e = hipEventSynchronize(d.ev_stg[(ngroups - 1) % kStageSlots])) != hipSuccess)
        return drain(hip_fail(e, "hipEventSynchronize"));
    copy_out(ngroups - 1);
    } catch (const std::exception& x) {
        return drain(set_status(FEC_ENOMEM, "staged batch path: %s", x.what()));
    }
    drain(FEC_OK);
    return set_status(FEC_OK);
}

// Run `coef` (r x k) over in -> out.  Device blocks are used in place; host
// blocks are staged (small calls: one pinned bounce buffer each way; large
// calls: the staged path).  Synchronous unless FEC_FLAG_ASYNC and every
// block is device memory.
int run_single(const uint8_t* coef, unsigned k, unsigned r, const gf* const* in, gf* const* out, size_t sz,
               void* stream_arg, unsigned flags) {
    if (!gpu_available()) return set_status(FEC_ENODEV, "no GPU visible to HIP (the engine has no CPU path)");
    thread_local Marshal t_m;  // reused: no allocation per call once its vectors have grown
    Marshal& m = t_m;
    if (flags & FEC_FLAG_HOST_MEMORY) {  // the caller vouches: every block is host memory
        for (unsigned j = 0; j < k; ++j)
            if (!in[j]) return set_status(FEC_EINVAL, "input block %u is NULL", j);
        for (unsigned i = 0; i < r; ++i)
            if (!out[i]) return set_status(FEC_EINVAL, "output block %u is NULL", i);
        m.zin.assign(in, in + k);
        m.zout.assign(out, out + r);
        m.in_host.clear();
        m.out_host.clear();
        for (unsigned j = 0; j < k; ++j) m.in_host.push_back(static_cast<int>(j));
        for (unsigned i = 0; i < r; ++i) m.out_host.push_back(static_cast<int>(i));
        m.all_pinned = false;
        if (hipGetDevice(&m.device) != hipSuccess) return set_status(FEC_ENODEV, "no current HIP device");
    } else if (classify(in, k, out, r, m)) {
        return t_status;
    }
    DeviceGuard guard(m.device);
    DevCtx* d = nullptr;
    if (dev_ctx(m.device, &d)) return t_status;
    hipStream_t st = (flags & FEC_FLAG_LIBRARY_STREAM) ? d->stream : static_cast<hipStream_t>(stream_arg);
    if (sz == 0 || r == 0) return set_status(FEC_OK);
    const size_t nhost = m.in_host.size() + m.out_host.size();
    const Config& cfg = config();
    hipError_t e;
    if (nhost == 0) {
        if (apply_matrix(coef, k, r, in, out, sz, 1, 0, 0, st)) return t_status;
        if (!(flags & FEC_FLAG_ASYNC) && (e = hipStreamSynchronize(st)) != hipSuccess)
            return hip_fail(e, "hipStreamSynchronize");
        return set_status(FEC_OK);
    }
    // Page-locked host blocks are read and written by the kernel itself over
    // PCIe (zero-copy): both link directions run at once with no staging
    // copies (K=3/M=10, 64 MiB: 21 GB/s of input vs 16.6 through a chunked
    // copy pipeline; tools/mb_host.hip).
    auto map_all = [&]() {
        bool ok = true;
        for (int i : m.in_host) ok = ok && (m.zin[i] = mapped_block(in[i], sz)) != nullptr;
        for (int i : m.out_host) ok = ok && (m.zout[i] = const_cast<uint8_t*>(mapped_block(out[i], sz))) != nullptr;
        return ok;
    };
    if (m.all_pinned && map_all()) {
        if (apply_matrix(coef, k, r, m.zin.data(), m.zout.data(), sz, 1, 0, 0, st)) return t_status;
        if (!(flags & FEC_FLAG_ASYNC) && (e = hipStreamSynchronize(st)) != hipSuccess)
            return hip_fail(e, "hipStreamSynchronize");
        return set_status(FEC_OK);
    }
    // large pageable blocks: staged through pinned slots by the host threads.
    // Calls whose kernel can use the bounce buffer in place (k <= 4, r <= 8)
    // stay on it up to Config::zc_limit: K=3/M=10 from bytes, 256 KiB stripes
    // (874 KB of host blocks) encode in 47-57 us there against 62-71 us staged
    // and decode in 30-35 against 45-52; 512 KiB stripes (1.75 MB) encode
    // 78-97 against 84-86 us (box-dependent: staged from 1.5 MiB) and decode
    // (1.05 MB) 49-56 against 61 us; 1 MiB stripes 186 against 159 us
    // (tools/archive/small_ab_inproc.py --set stage, profiles/r03_stage_ab.log).
    const bool zc_shape = k <= 4 && r <= 8;
    const size_t stage_from = zc_shape ? std::max(cfg.stage_min, cfg.zc_limit) : cfg.stage_min;
    if (sz * nhost > cfg.pack_limit || (sz * nhost > stage_from && sz >= kStageMinBlock))
        return run_staged(*d, coef, k, r, in, out, sz, m, st);

    // small call: pack the host inputs into the thread's pinned buffer.  Up to
    // Config::zc_limit bytes the kernel reads them and writes the host outputs
    // there in place over PCIe (no copy calls: 4 KiB K=3/M=10 encode 21.9 ->
    // 16.6 us per call, 128 KiB 46.8 -> 26.6 us); wide codes (and calls past
    // the limit) move the packed blocks with one H2D and one D2H copy.
    // Device-resident blocks are used in place.  Then unpack.
    m.din.assign(in, in + k);
    m.dout.assign(out, out + r);
    const size_t slot = align_up(sz, 256);
    const size_t nin = m.in_host.size(), nout = m.out_host.size();
    if (ensure_hbuf(*d, slot * (nin + nout))) return t_status;
    uint8_t* hb = static_cast<uint8_t*>(d->hbuf);  // free: the previous call on this thread synchronised
    // the copies run on this thread (on the host pool they measured slower at
    // every size this path serves: profiles/r02_host_lat_ab.log, r03_pool_ab.log)
    auto copy_blocks = [&](bool to_slot) {
        const size_t n = to_slot ? nin : nout;
        for (size_t q = 0; q < n; ++q) {
            uint8_t* sl = hb + slot * (to_slot ? q : nin + q);
            if (to_slot)
                std::memcpy(sl, in[m.in_host[q]], sz);
            else
                std::memcpy(out[m.out_host[q]], sl, sz);
        }
    };
    // Every block in the bounce buffer: its slots are 256-byte multiples, so
    // the kernel may run each row out to its next 128-byte line (whole 16-byte
    // units, no byte-wise tail: over PCIe each tail byte load is a round trip
    // of its own); the bytes past sz are never copied out.
    const size_t ksz = nhost == size_t(k) + r ? std::min(slot, align_up(sz, 128)) : sz;
    // The compact one-workgroup kernel takes the inputs inside its argument
    // block where they fit (kernels.hip OneJobInline): no copy into the bounce
    // buffer, no PCIe reads in the kernel.
    const bool one_shape = k <= 4 && r <= 8 && ksz % 16 == 0 && ksz <= 4096 && sz * nhost <= cfg.zc_limit;
    const bool inline_in = one_shape && nin == k && nhost == size_t(k) + r && one_inline_fits(k, ksz, sz);
    if (!inline_in) copy_blocks(true);
    // Zero-copy only for the register kernels (k <= 4, r <= 8), which issue
    // all their input loads at once: the wide-code kernels read inputs in
    // groups, each group a PCIe round trip of its own (K=20/M=60, 4 KiB stripe:
    // 40 us in the kernel over PCIe; tools/small_call_probe.py under
    // rocprofv3, profiles/r02_small_calls.log) -- except small packs, up to
    // kZcWideLimit: K=20/M=60 from bytes, 4 KiB stripes encode in 20.5 us in
    // place against 25.3 us with the copies, 64 KiB (197 KB of host blocks)
    // 44.7 against 47.9 us, but 128 KiB (393 KB) 63.8 against 57.9 us
    // (round-3 A/B, profiles/r03_zcwide_ab.log).  Fixed since round 4; the
    // GPU test test_medium_call_wait_modes runs K=10/M=16 on both sides of it.
    constexpr size_t kZcWideLimit = size_t(256) << 10;
    const bool zc_kernel = (k <= 4 && r <= 8) || sz * nhost <= kZcWideLimit;
    bool signalled = false;
    const bool zero_copy = sz * nhost <= cfg.zc_limit && zc_kernel;
    if (zero_copy) {
        uint8_t* hbd = static_cast<uint8_t*>(d->hbuf_dev);
        for (size_t q = 0; q < nin; ++q) m.din[m.in_host[q]] = hbd + slot * q;
        for (size_t q = 0; q < nout; ++q) m.dout[m.out_host[q]] = hbd + slot * (nin + q);
        if (one_shape) {
            // whole 16-byte units in one workgroup: the compact kernel
            // (kernels.hip matapply_one), which signals its own completion
            uint32_t* f = signal_slot(*d);
            ApplySpec a;
            a.coef = coef;
            a.coef_stride = k;
            a.k = k;
            a.r = r;
            a.in = m.din.data();
            a.out = m.dout.data();
            a.sz = ksz;
            a.nstripes = 1;
            a.in_sstride = a.out_sstride = 0;
            a.accumulate = false;
            ++t_launches;
            const hipError_t le = launch_one(a, st, f, f ? d->seq : 0, inline_in ? in : nullptr, sz);
            if (le != hipSuccess) return hip_fail(le, "launch_one");
            signalled = f != nullptr;
        } else {
            // one launch of at most one workgroup (k <= 4, r <= 8, sz <= 4 KiB): it
            // signals its own completion
            if (k <= 4 && r <= 8 && sz <= 4096)
                if (uint32_t* f = signal_slot(*d)) matapply_request_signal(f, d->seq);
            const unsigned launches0 = t_launches;
            const int st0 = apply_matrix(coef, k, r, m.din.data(), m.dout.data(), ksz, 1, 0, 0, st);
            // the kernel's signal covers the call only if it was its one launch
            signalled = st0 == FEC_OK && matapply_signal_used() && t_launches - launches0 == 1;
            matapply_request_signal(nullptr, 0);  // an unconsumed request must not reach a later launch
            if (st0) return t_status;
        }
    } else {
        if (ensure_dbuf(*d, slot * nhost)) return t_status;
        uint8_t* base = static_cast<uint8_t*>(d->dbuf);
        for (size_t q = 0; q < nin; ++q) m.din[m.in_host[q]] = base + slot * q;
        for (size_t q = 0; q < nout; ++q) m.dout[m.out_host[q]] = base + slot * (nin + q);
        if (nin && (e = hipMemcpyAsync(base, hb, slot * nin, hipMemcpyHostToDevice, st)) != hipSuccess)
            return hip_fail(e, "hipMemcpyAsync H2D");
        if (apply_matrix(coef, k, r, m.din.data(), m.dout.data(), ksz, 1, 0, 0, st)) return t_status;
        if (nout && (e = hipMemcpyAsync(hb + slot * nin, base + slot * nin, slot * nout, hipMemcpyDeviceToHost,
                                        st)) != hipSuccess)
            return hip_fail(e, "hipMemcpyAsync D2H");
    }
    if (!signalled && zero_copy) {
        // a zero-copy launch of several workgroups: the stream itself writes
        // the call's sequence number into the pinned completion word after the
        // kernel, and the thread spins on that (64 KiB K=3/M=10 encode 23.8 ->
        // 21.2 us, decode 19.1 -> 16.4 us in an interleaved A/B,
        // profiles/r03_wait_ab.log).  Not behind the copy path's D2H copy:
        // there it measured 6-7 us slower than hipStreamSynchronize.
        if (uint32_t* f = signal_slot(*d)) {
            if (hipStreamWriteValue32(st, f, d->seq, 0) == hipSuccess)
                signalled = true;
            else
                (void)hipGetLastError();
        }
    }
    t_last_wait = signalled ? 1 : 0;
    if ((e = signalled ? wait_signal(*d, st) : hipStreamSynchronize(st)) != hipSuccess)
        return hip_fail(e, "hipStreamSynchronize");
    copy_blocks(false);
    return set_status(FEC_OK);
}

int check_block_nums(const fec_t* code, const unsigned* nums, size_t num) {
    if (num && !nums) return set_status(FEC_EINVAL, "block_nums is NULL");
    for (size_t i = 0; i < num; ++i)
        if (nums[i] >= code->n)
            return set_status(FEC_EINVAL, "block number %u out of range (n = %u)", nums[i], unsigned(code->n));
    return FEC_OK;
}

// The decode matrix rows to apply (r x k, into `rows`): the missing
// primaries' (ascending), or with all_primaries every primary's (a present
// primary's row is a unit vector: the output is a copy, so the k outputs are
// the stripe in order).
int decode_rows(const fec_t* code, const unsigned* index, std::vector<uint8_t>& rows, unsigned& r,
                bool all_primaries = false) {
    const unsigned k = code->k;
    if (!index) return set_status(FEC_EINVAL, "index is NULL");
    unsigned char seen[256] = {};
    for (unsigned i = 0; i < k; ++i) {
        if (index[i] >= code->n)
            return set_status(FEC_EINVAL, "block number %u out of range (n = %u)", index[i], unsigned(code->n));
        if (seen[index[i]]) return set_status(FEC_EINVAL, "duplicate block number %u", index[i]);
        seen[index[i]] = 1;
        if (index[i] < k && index[i] != i)
            return set_status(FEC_EINVAL, "primary block %u must be at slot %u, found at slot %u", index[i], index[i], i);
    }
    // The inverse is O(k^3) on the host (255 x 255 with 128 secondaries:
    // ~0.8 ms, more than the kernel), and batches of stripes are decoded from
    // the same blocks call after call, so each thread keeps its last few
    // decode matrices.  The key is (k, index): the encoding matrix's row b
    // depends on k and b only, not on n (zfec/fec.c:456-469; checked against
    // the reference).
    struct Cached {
        unsigned k = 0;
        bool all = false;
        std::vector<unsigned> idx;
        std::vector<uint8_t> rows;
        unsigned r = 0;
    };
    constexpr int kCache = 8;
    thread_local Cached cache[kCache];
    thread_local unsigned next = 0;
    for (const Cached& c : cache)
        if (c.k == k && c.all == all_primaries && std::equal(index, index + k, c.idx.begin(), c.idx.end())) {
            rows.assign(c.rows.begin(), c.rows.end());
            r = c.r;
            return FEC_OK;
        }
    thread_local std::vector<uint8_t> dec;
    dec.resize(size_t(k) * k);
    if (!build_decode_matrix(code->enc_matrix, k, index, dec.data()))
        return set_status(FEC_ESINGULAR, "decode matrix is singular");
    rows.clear();
    r = 0;
    for (unsigned i = 0; i < k; ++i) {
        if (index[i] < k && !all_primaries) continue;
        rows.insert(rows.end(), dec.begin() + size_t(i) * k, dec.begin() + size_t(i + 1) * k);
        ++r;
    }
    Cached& c = cache[next++ % kCache];
    c.k = k;
    c.all = all_primaries;
    c.idx.assign(index, index + k);
    c.rows.assign(rows.begin(), rows.end());
    c.r = r;
    return FEC_OK;
}

// The encoding matrix rows of block_nums (num x k): consecutive ascending
// numbers are one contiguous run of enc_matrix (used in place), others are
// gathered into the thread's buffer.
const uint8_t* encode_rows(const fec_t* code, const unsigned* nums, size_t num) {
    const unsigned k = code->k;
    bool run = true;
    for (size_t i = 1; i < num && run; ++i) run = nums[i] == nums[0] + i;
    if (run) return code->enc_matrix + size_t(nums[0]) * k;
    thread_local std::vector<uint8_t> rows;
    rows.resize(num * k);
    for (size_t i = 0; i < num; ++i) std::memcpy(&rows[i * k], code->enc_matrix + size_t(nums[i]) * k, k);
    return rows.data();
}

}  // namespace
}  // namespace zfec_hip

using namespace zfec_hip;

// ============================================================================
// Part 1: zfec/fec.h drop-in
// ============================================================================

FEC_API void fec_init(void) {
    field_init();
    set_status(FEC_OK);
}

namespace {
void prefetch_rows(const uint8_t* coef, unsigned k, unsigned r);  // below, with prepare_rows
}

FEC_API fec_t* fec_new(unsigned short k, unsigned short m) {
    if (!field_ready()) {  // zfec/fec.c:442-444
        set_status(FEC_EUNINIT, "fec_init() has not been called");
        return nullptr;
    }
    if (k < 1 || m < 1 || m > 256 || k > m) {  // zfec/fec.c:437-440 (asserts there)
        set_status(FEC_EINVAL, "invalid code parameters k=%u m=%u", unsigned(k), unsigned(m));
        return nullptr;
    }
    fec_t* p = static_cast<fec_t*>(std::calloc(1, sizeof(fec_t)));
    gf* enc = static_cast<gf*>(std::malloc(size_t(k) * m));
    if (!p || !enc) {
        std::free(p);
        std::free(enc);
        set_status(FEC_ENOMEM, "out of host memory");
        return nullptr;
    }
    build_encoding_matrix(k, m, enc);
    p->k = k;
    p->n = m;
    p->enc_matrix = enc;
    p->priv = nullptr;
    p->magic = magic_of(p);
    // the full encode's compiled kernels, where an earlier process left them in
    // the JIT disk cache: loaded in the background, so this code's first large
    // encode can run them (bitslice.hpp jit_prefetch; no compile, no wait)
    prefetch_rows(enc + size_t(k) * k, k, static_cast<unsigned>(m - k));
    set_status(FEC_OK);
    return p;
}

FEC_API void fec_free(fec_t* p) {
    if (!p) return;
    if (!valid_code(p)) {  // zfec/fec.c:425 asserts; we refuse and report
        set_status(FEC_EINVAL, "fec_free: bad magic");
        return;
    }
    p->magic = 0;
    std::free(p->enc_matrix);
    std::free(p);
    set_status(FEC_OK);
}

FEC_API int fec_encode_ex(const fec_t* code, const gf* const* src, gf* const* fecs, const unsigned* block_nums,
                          size_t num_block_nums, size_t sz, void* stream, unsigned flags) {
    if (!valid_code(code)) return set_status(FEC_EINVAL, "invalid fec_t");
    if (check_block_nums(code, block_nums, num_block_nums)) return t_status;
    if (num_block_nums == 0) return set_status(FEC_OK);
    if (!src || !fecs) return set_status(FEC_EINVAL, "NULL block array");
    return guarded([&] {
        const uint8_t* rows = encode_rows(code, block_nums, num_block_nums);
        return run_single(rows, code->k, static_cast<unsigned>(num_block_nums), src, fecs, sz, stream, flags);
    });
}

namespace {
// fec.h's fec_encode / fec_decode return void and their callers (the
// reference's _fecmodule.c, the Haskell binding) never ask for a status, so a
// failure there would hand back unwritten output buffers in silence.  The
// first failure of each entry point is reported on stderr (once per process;
// ZFEC_HIP_QUIET=1 silences it); fec_last_status() still holds every one.
void report_void_failure(const char* fn, int st) {
    static std::atomic<int> reported[2] = {{0}, {0}};
    std::atomic<int>& once = reported[fn[4] == 'd' ? 1 : 0];
    if (config().quiet || once.exchange(1) != 0) return;
    fprintf(stderr,
            "zfec_hip: %s failed (status %d: %s); its output blocks are not valid.  Further failures of %s are "
            "not reported here; fec_last_status() / fec_last_error_message() give each call's status.\n",
            fn, st, t_msg, fn);
    fflush(stderr);
}
}  // namespace

FEC_API void fec_encode(const fec_t* code, const gf* const* src, gf* const* fecs, const unsigned* block_nums,
                        size_t num_block_nums, size_t sz) {
    const int st = fec_encode_ex(code, src, fecs, block_nums, num_block_nums, sz, nullptr, FEC_FLAG_LIBRARY_STREAM);
    if (st != FEC_OK) report_void_failure("fec_encode", st);
}

FEC_API int fec_decode_ex(const fec_t* code, const gf* const* inpkts, gf* const* outpkts, const unsigned* index,
                          size_t sz, void* stream, unsigned flags) {
    if (!valid_code(code)) return set_status(FEC_EINVAL, "invalid fec_t");
    thread_local std::vector<uint8_t> rows;
    unsigned r = 0;
    if (decode_rows(code, index, rows, r, (flags & FEC_FLAG_ALL_PRIMARIES) != 0)) return t_status;
    if (r == 0) return set_status(FEC_OK);
    if (!inpkts || !outpkts) return set_status(FEC_EINVAL, "NULL block array");
    return guarded([&] { return run_single(rows.data(), code->k, r, inpkts, outpkts, sz, stream, flags); });
}

FEC_API void fec_decode(const fec_t* code, const gf* const* inpkts, gf* const* outpkts, const unsigned* index,
                        size_t sz) {
    const int st = fec_decode_ex(code, inpkts, outpkts, index, sz, nullptr, FEC_FLAG_LIBRARY_STREAM);
    if (st != FEC_OK) report_void_failure("fec_decode", st);
}

FEC_API void build_decode_matrix_into_space(const fec_t* code, const unsigned* index, const unsigned k, gf* matrix) {
    if (!valid_code(code) || k != code->k || !index || !matrix) {
        set_status(FEC_EINVAL, "build_decode_matrix_into_space: bad arguments");
        return;
    }
    for (unsigned i = 0; i < k; ++i)
        if (index[i] >= code->n) {
            set_status(FEC_EINVAL, "block number %u out of range", index[i]);
            return;
        }
    if (!build_decode_matrix(code->enc_matrix, k, index, matrix))
        set_status(FEC_ESINGULAR, "decode matrix is singular");
    else
        set_status(FEC_OK);
}

FEC_API void _invert_vdm(gf* src, unsigned k) {
    field_init();
    invert_vandermonde(src, k);
}

// ============================================================================
// Part 2: extensions
// ============================================================================

FEC_API int fec_last_status(void) { return t_status; }
FEC_API const char* fec_last_error_message(void) { return t_msg; }

FEC_API int fec_device_count(void) { return gpu_available(); }

FEC_API void* fec_host_alloc(size_t bytes) {
    if (!gpu_available()) {
        set_status(FEC_ENODEV, "no GPU visible to HIP");
        return nullptr;
    }
    void* p = nullptr;
    hipError_t e = hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) {
        set_status(FEC_ENOMEM, "hipHostMalloc(%zu): %s", bytes, hipGetErrorString(e));
        return nullptr;
    }
    set_status(FEC_OK);
    return p;
}

FEC_API void fec_host_free(void* p) {
    if (p) (void)hipHostFree(p);
    set_status(FEC_OK);
}

FEC_API const char* fec_version(void) { return "zfec-hip 0.1.0 (gfx950)"; }

FEC_API const char* fec_kernel_name(unsigned k, unsigned r) {
    if (k == 0 || r == 0 || k > static_cast<unsigned>(kMaxIn) || r > static_cast<unsigned>(kMaxOut)) return "split";
    return matapply_variant_name(k, r, false);
}

FEC_API const char* fec_last_kernel_name(void) { return matapply_last_kernel(); }

FEC_API int fec_jit_mode(int mode) {
    const int prev = static_cast<int>(jit_mode());
    if (mode >= kJitOff && mode <= kJitForce) set_jit_mode(static_cast<JitMode>(mode));
    set_status(FEC_OK);
    return prev;
}

FEC_API int fec_generic_mode(int mode) {
    const int prev = generic_mode();
    if (mode >= 0 && mode <= 2) set_generic_mode(mode);
    set_status(FEC_OK);
    return prev;
}

FEC_API int fec_jit_wait(void) {
    set_status(FEC_OK);
    return jit_wait();
}

FEC_API int fec_reload_config(void) {
    reload_config();
    return set_status(FEC_OK);
}

FEC_API int fec_last_wait(void) { return t_last_wait; }

namespace {
// Compile the specialised kernels apply_matrix_range would launch for this
// r x k matrix in large launches: its row groups of one launch each (the same
// near-equal groups).  Groups past kJitMaxCoef coefficients run on
// matapply_bsg and need no compile.
int prepare_rows(const uint8_t* coef, unsigned k, unsigned r) {
    if (r == 0) return set_status(FEC_OK);
    const bool wide = k > static_cast<unsigned>(kMaxIn);
    const unsigned rmax =
        wide ? static_cast<unsigned>(kMaxOut) : std::max<unsigned>(1, std::min<unsigned>(kMaxOut, kMaxCoef / k));
    const unsigned ngroups = (r + rmax - 1) / rmax;
    for (unsigned g = 0; g < ngroups; ++g) {
        const unsigned i0 = g * r / ngroups, rg = (g + 1) * r / ngroups - i0;
        if (k * rg > kJitMaxCoef) continue;
        if (jit_prepare(coef + size_t(i0) * k, k, rg) != 0)
            return set_status(FEC_EHIP, "JIT compile failed: %s", jit_last_error().c_str());
    }
    return set_status(FEC_OK);
}
}  // namespace

namespace {
// jit_prefetch for the row groups prepare_rows would compile.
void prefetch_rows(const uint8_t* coef, unsigned k, unsigned r) {
    if (r == 0 || jit_mode() != kJitAuto) return;
    const bool wide = k > static_cast<unsigned>(kMaxIn);
    const unsigned rmax =
        wide ? static_cast<unsigned>(kMaxOut) : std::max<unsigned>(1, std::min<unsigned>(kMaxOut, kMaxCoef / k));
    const unsigned ngroups = (r + rmax - 1) / rmax;
    for (unsigned g = 0; g < ngroups; ++g) {
        const unsigned i0 = g * r / ngroups, rg = (g + 1) * r / ngroups - i0;
        if (k * rg <= kJitMaxCoef) jit_prefetch(coef + size_t(i0) * k, k, rg);
    }
}
}  // namespace

FEC_API int fec_jit_prepare_encode(const fec_t* code, const unsigned* block_nums, size_t num_block_nums) {
    if (!valid_code(code)) return set_status(FEC_EINVAL, "invalid fec_t");
    if (check_block_nums(code, block_nums, num_block_nums)) return t_status;
    if (num_block_nums == 0) return set_status(FEC_OK);
    return prepare_rows(encode_rows(code, block_nums, num_block_nums), code->k, static_cast<unsigned>(num_block_nums));
}

FEC_API int fec_jit_prepare_decode(const fec_t* code, const unsigned* index, unsigned flags) {
    if (!valid_code(code)) return set_status(FEC_EINVAL, "invalid fec_t");
    std::vector<uint8_t> rows;
    unsigned r = 0;
    if (decode_rows(code, index, rows, r, (flags & FEC_FLAG_ALL_PRIMARIES) != 0)) return t_status;
    return prepare_rows(rows.data(), code->k, r);
}

namespace {
// The launch geometry of a batched call on device (or page-locked) memory:
// updates sz and nstripes in place.
void batch_geometry(unsigned k, unsigned r, size_t sbs, size_t sss, size_t dbs, size_t dss, unsigned flags, size_t& sz,
                    size_t& nstripes) {
    // Block-major batches (stripes packed back to back inside each block array,
    // both strides == sz) are one stripe of nstripes * sz bytes: output byte x
    // depends only on byte x of the inputs (zfec/fec.c:494-503, :547-556), so
    // one long-stream launch replaces the walk over short rows.
    // FEC_FLAG_ROW_PADDING: run the rows out to a whole 128-byte line where the
    // strides leave room.  A row ending mid-line leaves a partly written line
    // that HBM completes with a read-modify-write: 10^6 K=3/M=10 stripes of
    // 1366-byte blocks in 1536-byte rows encode in 2.91 ms, of 1408-byte blocks
    // in 2.55 ms (tools/archive/grid_probe.py, profiles/r01_grid_probe_sz.log).
    // `grant`: bytes past a row's start the flag lets us touch (per row).
    size_t grant = sz;
    if (flags & FEC_FLAG_ROW_PADDING) {
        const size_t padded = (sz + 127) / 128 * 128;
        const bool room = sbs >= padded && dbs >= padded && (nstripes == 1 || (sss >= (k - 1) * sbs + padded &&
                                                                                dss >= (r - 1) * dbs + padded));
        if (room) grant = padded;
    }
    if (nstripes > 1 && sss == sz && dss == sz && sz <= SIZE_MAX / nstripes) {
        // the collapsed row may run out to its own next line only inside the
        // last stripe's grant: (nstripes - 1) * sz + grant
        const size_t len = sz * nstripes, padded = (len + 127) / 128 * 128;
        sz = padded <= len - sz + grant ? padded : len;
        nstripes = 1;
    } else {
        sz = grant;
    }
}

int run_batch(const fec_t* code, const uint8_t* coef, unsigned r, const gf* src, size_t sbs, size_t sss, gf* dst,
              size_t dbs, size_t dss, size_t sz, size_t nstripes, void* stream, unsigned flags) {
    const unsigned k = code->k;
    if (!gpu_available()) return set_status(FEC_ENODEV, "no GPU visible to HIP (the engine has no CPU path)");
    if (!src || !dst) return set_status(FEC_EINVAL, "NULL buffer");
    // one pointer query per side: device memory (its device), or host memory
    const BatchBuf bufs[2] = {{src, (nstripes - 1) * sss + (k - 1) * sbs + sz, "src"},
                              {dst, (nstripes - 1) * dss + (r - 1) * dbs + sz, "dst"}};
    BatchMem m;
    if (resolve_batch(m, nullptr, bufs, 2, nullptr, -1, stream, flags, nullptr)) return t_status;
    // pageable host memory on either side: staged through pinned slots
    // (synchronous whatever the flags; FEC_FLAG_ROW_PADDING does not apply)
    if (sz && nstripes && r && (!m.z[0] || !m.z[1]))
        return run_batch_staged(*m.d, coef, k, r, m.z[0] ? m.z[0] : src, sbs, sss, !m.z[0],
                                m.z[1] ? const_cast<gf*>(m.z[1]) : dst, dbs, dss, !m.z[1], sz, nstripes, m.st);
    batch_geometry(k, r, sbs, sss, dbs, dss, flags, sz, nstripes);
    // page-locked host memory (zero-copy) has to cover the rows as the geometry lengthened them
    if (m.bdev[0] < 0 && !(m.z[0] = mapped_block(src, (nstripes - 1) * sss + (k - 1) * sbs + sz)))
        return set_status(FEC_EINVAL, "batched entry points take device or page-locked host memory");
    if (m.bdev[1] < 0 && !(m.z[1] = mapped_block(dst, (nstripes - 1) * dss + (r - 1) * dbs + sz)))
        return set_status(FEC_EINVAL, "batched entry points take device or page-locked host memory");
    const uint8_t* in[kMaxWideIn];
    uint8_t* out[kMaxWideIn];
    for (unsigned j = 0; j < k; ++j) in[j] = m.z[0] + j * sbs;
    for (unsigned i = 0; i < r; ++i) out[i] = const_cast<gf*>(m.z[1]) + i * dbs;
    if (apply_matrix(coef, k, r, in, out, sz, nstripes, sss, dss, m.st)) return t_status;
    if (!(flags & FEC_FLAG_ASYNC)) {
        hipError_t e = hipStreamSynchronize(m.st);
        if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
    }
    return set_status(FEC_OK);
}
}  // namespace

FEC_API int fec_encode_batch(const fec_t* code, const gf* src, size_t src_block_stride, size_t src_stripe_stride,
                             gf* dst, size_t dst_block_stride, size_t dst_stripe_stride, const unsigned* block_nums,
                             size_t num_block_nums, size_t sz, size_t nstripes, void* stream, unsigned flags) {
    if (!valid_code(code)) return set_status(FEC_EINVAL, "invalid fec_t");
    if (check_block_nums(code, block_nums, num_block_nums)) return t_status;
    if (num_block_nums == 0 || sz == 0 || nstripes == 0) return set_status(FEC_OK);
    return guarded([&] {
        return run_batch(code, encode_rows(code, block_nums, num_block_nums), static_cast<unsigned>(num_block_nums),
                         src, src_block_stride, src_stripe_stride, dst, dst_block_stride, dst_stripe_stride, sz,
                         nstripes, stream, flags);
    });
}

FEC_API int fec_decode_batch(const fec_t* code, const gf* src, size_t src_block_stride, size_t src_stripe_stride,
                             gf* dst, size_t dst_block_stride, size_t dst_stripe_stride, const unsigned* index,
                             size_t sz, size_t nstripes, void* stream, unsigned flags) {
    if (!valid_code(code)) return set_status(FEC_EINVAL, "invalid fec_t");
    thread_local std::vector<uint8_t> rows;
    unsigned r = 0;
    if (decode_rows(code, index, rows, r, (flags & FEC_FLAG_ALL_PRIMARIES) != 0)) return t_status;
    if (r == 0 || sz == 0 || nstripes == 0) return set_status(FEC_OK);
    return guarded([&] {
        return run_batch(code, rows.data(), r, src, src_block_stride, src_stripe_stride, dst, dst_block_stride,
                         dst_stripe_stride, sz, nstripes, stream, flags);
    });
}

// ---- ragged batches: a size per stripe ------------------------------------------------
namespace {
constexpr char kCaptureRagged[] = "the call stages per call through slots the library reuses";

struct RaggedCall {
    const char* fn;
    const gf* src;
    size_t src_bytes, sbs;
    const unsigned long long* soff;
    gf* dst;
    size_t dst_bytes, dbs;
    const unsigned long long* doff;
    const unsigned long long* sizes;
    size_t nstripes;
    void* stream;
    unsigned flags;
};

int ragged_null(const RaggedCall& c, const void* nums, const char* nums_name) {
    const struct {
        const void* p;
        const char* name;
    } args[] = {{c.src, "src"},          {c.dst, "dst"}, {c.sizes, "sizes"}, {c.soff, "src_offsets"},
                {c.doff, "dst_offsets"}, {nums, nums_name}};
    for (const auto& a : args)
        if (!a.p) return set_status(FEC_EINVAL, "%s: %s is NULL", c.fn, a.name);
    return FEC_OK;
}

// The descriptors of a ragged call, over one arena (the scrub calls) or two:
// the arrays where the host reads them -- the caller's own, or fetch_desc's
// copies -- and each arena as the messages name it.
struct RaggedArena {
    const char *name, *off_name, *bytes_name;
    size_t bytes, bstride, rows;  // rows: blocks per stripe on this side
};
struct RaggedArgs {
    const char* fn;
    const char* mixed_kinds;  // the message for descriptor arrays of mixed memory kinds (one %s: fn)
    int na;                   // arenas: 1 or 2
    RaggedArena a[2];
    size_t nstripes;
    const unsigned long long* sizes;
    const unsigned long long* off[2];
    const unsigned* ids = nullptr;  // the repair's pattern ids, where given
};

RaggedArgs ragged_args(const RaggedCall& c, unsigned k, unsigned r) {
    return RaggedArgs{c.fn,
                      "%s: sizes, src_offsets and dst_offsets are of mixed memory kinds: all three in host memory, or "
                      "all three in device memory on the blocks' device",
                      2, {{"src", "src_offsets", "src_bytes", c.src_bytes, c.sbs, k},
                                {"dst", "dst_offsets", "dst_bytes", c.dst_bytes, c.dbs, r}},
                      c.nstripes, c.sizes, {c.soff, c.doff}};
}

// Whether stripe s fits every arena (kernels.hpp ragged_fits); *which: the first it does not.
bool ragged_stripe_fits(const RaggedArgs& d, size_t s, int* which = nullptr) {
    const uint64_t sz = d.sizes[s];
    for (int i = 0; i < d.na; ++i)
        if (!ragged_fits(d.off[i][s], d.a[i].bstride ? d.a[i].bstride : sz, static_cast<uint32_t>(d.a[i].rows), sz,
                         d.a[i].bytes)) {
            if (which) *which = i;
            return false;
        }
    return true;
}

// The checks of a ragged call that follow its block numbers, in the header's
// order: the stripe count and the memory kind of the descriptor arrays
// (check_ragged_kinds; *ddev: their device, -1 host memory), then with host
// arrays every stripe's fit (check_ragged_fit).  fec_repair_batch_ragged checks
// its host-side ids between the two.
int check_ragged_kinds(const RaggedArgs& d, int* ddev) {
    if (uint64_t(d.nstripes) >= (1ull << 32))
        return set_status(FEC_EINVAL, "%s: %zu stripes: a call takes fewer than 2^32", d.fn, d.nstripes);
    int dv[3] = {-1, -1, -1};
    if (gpu_available() && d.nstripes) {
        dv[0] = pointer_device(d.sizes);
        for (int i = 0; i < d.na; ++i) dv[1 + i] = pointer_device(d.off[i]);
    }
    if (dv[0] != dv[1] || (d.na == 2 && dv[0] != dv[2])) return set_status(FEC_EINVAL, d.mixed_kinds, d.fn);
    *ddev = dv[0];
    return FEC_OK;
}

int check_ragged_fit(const RaggedArgs& d, int ddev) {
    if (ddev < 0)
        for (size_t s = 0; s < d.nstripes; ++s) {
            int i = 0;
            if (d.sizes[s] && !ragged_stripe_fits(d, s, &i)) {
                const RaggedArena& a = d.a[i];
                return set_status(FEC_EINVAL, "%s: stripe %zu does not fit %s: offset %llu, %zu rows %llu apart, size "
                                              "%llu, %s %zu", d.fn, s, a.name, d.off[i][s], a.rows,
                                  static_cast<unsigned long long>(a.bstride ? a.bstride : d.sizes[s]), d.sizes[s],
                                  a.bytes_name, a.bytes);
            }
        }
    return FEC_OK;
}

int check_ragged(const RaggedArgs& d, int* ddev) {
    if (check_ragged_kinds(d, ddev)) return t_status;
    return check_ragged_fit(d, *ddev);
}

// Descriptor arrays in device memory (ddev >= 0), and pattern ids there (idev
// >= 0), brought to the host for the calls that cut runs: copies on `st` into
// the thread's buffers and one synchronise; d then reads the copies.
int fetch_desc(RaggedArgs& d, int ddev, int idev, hipStream_t st) {
    thread_local std::vector<unsigned long long> hd;
    thread_local std::vector<unsigned> hids;
    const size_t ns = d.nstripes;
    hipError_t e;
    if (ddev >= 0) {
        hd.resize((1 + d.na) * ns);
        const unsigned long long* from[3] = {d.sizes, d.off[0], d.off[1]};
        for (int i = 0; i < 1 + d.na; ++i)
            if ((e = hipMemcpyAsync(&hd[i * ns], from[i], ns * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                    st)) != hipSuccess)
                return hip_fail(e, "hipMemcpyAsync D2H (descriptor arrays)");
        d.sizes = hd.data();
        for (int i = 0; i < d.na; ++i) d.off[i] = d.sizes + (1 + i) * ns;
    }
    if (d.ids && idev >= 0) {
        hids.resize(ns);
        if ((e = hipMemcpyAsync(hids.data(), d.ids, ns * sizeof(unsigned), hipMemcpyDeviceToHost, st)) != hipSuccess)
            return hip_fail(e, "hipMemcpyAsync D2H (pattern_of)");
        d.ids = hids.data();
    }
    if ((ddev >= 0 || (d.ids && idev >= 0)) && (e = hipStreamSynchronize(st)) != hipSuccess)
        return hip_fail(e, "hipStreamSynchronize");
    return FEC_OK;
}

// Maximal runs [s0, s1) of consecutive stripes that are live(s), have one size,
// are same(s0, s) and whose offsets each advance by a constant: each one
// uniform batched call.  run(s0, s1, step) with the offset steps (0 for a run
// of one); a stripe that is not live is passed over.
template <class Live, class Same, class Run>
int for_each_ragged_run(const RaggedArgs& d, Live live, Same same, Run run) {
    const size_t ns = d.nstripes;
    for (size_t s0 = 0; s0 < ns;) {
        if (!live(s0)) {
            ++s0;
            continue;
        }
        size_t s1 = s0 + 1, step[2] = {0, 0};
        // stripe s follows s - 1 at a rising offset in every arena, and belongs to the run of s0
        const auto joins = [&](size_t s) {
            for (int i = 0; i < d.na; ++i)
                if (d.off[i][s] <= d.off[i][s - 1]) return false;
            return d.sizes[s] == d.sizes[s0] && same(s0, s) && live(s);
        };
        const auto in_step = [&](size_t s) {
            for (int i = 0; i < d.na; ++i)
                if (d.off[i][s] - d.off[i][s - 1] != step[i]) return false;
            return true;
        };
        if (s1 < ns && joins(s1)) {
            for (int i = 0; i < d.na; ++i) step[i] = d.off[i][s1] - d.off[i][s0];
            ++s1;
            while (s1 < ns && joins(s1) && in_step(s1)) ++s1;
        }
        if (run(s0, s1, step)) return t_status;
        s0 = s1;
    }
    return FEC_OK;
}

int run_ragged(const RaggedCall& c, const fec_t* code, const uint8_t* coef, unsigned r, int ddev) {
    const unsigned k = code->k;
    const size_t ns = c.nstripes;
    // device memory on one device, or page-locked host memory (read and written in place)
    const BatchBuf bufs[2] = {{c.src, c.src_bytes, "src"}, {c.dst, c.dst_bytes, "dst"}};
    BatchMem mem;
    if (resolve_batch(mem, c.fn, bufs, 2, "sizes", ddev, c.stream, c.flags, kCaptureRagged)) return t_status;
    hipStream_t st = mem.st;
    hipError_t e;
    if (k <= kMixedMaxK) {
        RaggedSpec g;
        g.k = k;
        g.r = r;
        g.coef = coef;
        g.in = mem.z[0];
        g.out = const_cast<gf*>(mem.z[1]);
        g.in_bytes = c.src_bytes;
        g.out_bytes = c.dst_bytes;
        g.in_bstride = c.sbs;
        g.out_bstride = c.dbs;
        g.sizes = reinterpret_cast<const uint64_t*>(c.sizes);
        g.in_off = reinterpret_cast<const uint64_t*>(c.soff);
        g.out_off = reinterpret_cast<const uint64_t*>(c.doff);
        g.desc_host = ddev < 0;
        g.nstripes = ns;
        ++t_launches;
        if ((e = launch_ragged(g, st)) != hipSuccess) return hip_fail(e, "launch_ragged");
    } else {
        // wider codes: runs of consecutive stripes of one size whose two offsets
        // each advance by a constant, each run one shared-matrix batched launch
        RaggedArgs d = ragged_args(c, k, r);
        if (fetch_desc(d, ddev, -1, st)) return t_status;
        const unsigned jf = (c.flags & FEC_FLAG_LIBRARY_STREAM) | FEC_FLAG_ASYNC;
        // not live: empty, or (device-side arrays) it does not fit: neither read nor written
        if (for_each_ragged_run(
                d, [&](size_t s) { return d.sizes[s] && ragged_stripe_fits(d, s); }, [](size_t, size_t) { return true; },
                [&](size_t s0, size_t s1, const size_t* step) {
                    const size_t sz = d.sizes[s0];
                    return run_batch(code, coef, r, c.src + d.off[0][s0], c.sbs ? c.sbs : sz, step[0],
                                     c.dst + d.off[1][s0], c.dbs ? c.dbs : sz, step[1], sz, s1 - s0, c.stream, jf);
                }))
            return t_status;
    }
    if (!(c.flags & FEC_FLAG_ASYNC) && (e = hipStreamSynchronize(st)) != hipSuccess)
        return hip_fail(e, "hipStreamSynchronize");
    return set_status(FEC_OK);
}

int no_gpu() { return set_status(FEC_ENODEV, "no GPU visible to HIP (the engine has no CPU path)"); }
}  // namespace

FEC_API int fec_ragged_units(const unsigned long long* sizes, size_t nstripes, unsigned long long* ustart) {
    if ((!sizes && nstripes) || !ustart) return set_status(FEC_EINVAL, "fec_ragged_units: NULL argument");
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "8-byte descriptor words");
    ragged_units(reinterpret_cast<const uint64_t*>(sizes), nstripes, reinterpret_cast<uint64_t*>(ustart));
    return set_status(FEC_OK);
}

FEC_API int fec_encode_batch_ragged(const fec_t* code, const gf* src, size_t src_bytes, size_t src_block_stride,
                                    const unsigned long long* src_offsets, gf* dst, size_t dst_bytes,
                                    size_t dst_block_stride, const unsigned long long* dst_offsets,
                                    const unsigned long long* sizes, const unsigned* block_nums,
                                    size_t num_block_nums, size_t nstripes, void* stream, unsigned flags) {
    const RaggedCall c{"fec_encode_batch_ragged", src,         src_bytes, src_block_stride, src_offsets, dst,
                       dst_bytes,                 dst_block_stride, dst_offsets, sizes,     nstripes,    stream,
                       flags};
    if (!valid_code(code)) return set_status(FEC_EINVAL, "invalid fec_t");
    if (ragged_null(c, block_nums, "block_nums")) return t_status;
    if (num_block_nums == 0) return set_status(FEC_EINVAL, "%s: num_block_nums is 0", c.fn);
    for (size_t i = 0; i < num_block_nums; ++i)
        if (block_nums[i] >= code->n)
            return set_status(FEC_EINVAL, "%s: block number %u out of range (n = %u)", c.fn, block_nums[i],
                              unsigned(code->n));
    if (nstripes == 0) return set_status(FEC_OK);
    return guarded([&] {
        const unsigned r = static_cast<unsigned>(num_block_nums);
        int ddev = -1;
        if (check_ragged(ragged_args(c, code->k, r), &ddev)) return t_status;
        if (!gpu_available()) return no_gpu();
        return run_ragged(c, code, encode_rows(code, block_nums, num_block_nums), r, ddev);
    });
}

FEC_API int fec_decode_batch_ragged(const fec_t* code, const gf* src, size_t src_bytes, size_t src_block_stride,
                                    const unsigned long long* src_offsets, gf* dst, size_t dst_bytes,
                                    size_t dst_block_stride, const unsigned long long* dst_offsets,
                                    const unsigned long long* sizes, const unsigned* index, size_t nstripes,
                                    void* stream, unsigned flags) {
    const RaggedCall c{"fec_decode_batch_ragged", src,         src_bytes, src_block_stride, src_offsets, dst,
                       dst_bytes,                 dst_block_stride, dst_offsets, sizes,     nstripes,    stream,
                       flags};
    if (!valid_code(code)) return set_status(FEC_EINVAL, "invalid fec_t");
    if (ragged_null(c, index, "index")) return t_status;
    return guarded([&] {
        thread_local std::vector<uint8_t> rows;
        unsigned r = 0;
        if (decode_rows(code, index, rows, r, (flags & FEC_FLAG_ALL_PRIMARIES) != 0)) {
            const std::string msg = t_msg;  // fec_decode_batch's checks, named as this call's
            return set_status(t_status, "%s: %s", c.fn, msg.c_str());
        }
        if (nstripes == 0) return set_status(FEC_OK);
        int ddev = -1;
        if (check_ragged(ragged_args(c, code->k, r), &ddev)) return t_status;
        if (r == 0) return set_status(FEC_OK);  // no primary is missing: nothing to recover
        if (!gpu_available()) return no_gpu();
        return run_ragged(c, code, rows.data(), r, ddev);
    });
}

// ---- batched decode, a pattern per stripe ------------------------------------------
namespace {
// A pattern's k block numbers: each < n, all distinct.  `p`: its number, for the message.
int check_pattern(const fec_t* code, const unsigned* pat, size_t p) {
    unsigned char seen[256] = {};
    for (unsigned j = 0; j < code->k; ++j) {
        if (pat[j] >= code->n)
            return set_status(FEC_EINVAL, "pattern %zu: block number %u out of range (n = %u)", p, pat[j],
                              unsigned(code->n));
        if (seen[pat[j]]) return set_status(FEC_EINVAL, "pattern %zu: duplicate block number %u", p, pat[j]);
        seen[pat[j]] = 1;
    }
    return FEC_OK;
}

// The k x k matrix that yields the k primaries from slots holding the blocks
// pattern[0..k): the inverse of the matrix whose row j is enc_matrix's row
// pattern[j] (a primary's row there is its unit vector).  Any slot order.
int mixed_rows(const fec_t* code, const unsigned* pat, uint8_t* rows) {
    const unsigned k = code->k;
    for (unsigned j = 0; j < k; ++j) std::memcpy(rows + size_t(j) * k, code->enc_matrix + size_t(pat[j]) * k, k);
    if (!invert_matrix(rows, k)) return set_status(FEC_ESINGULAR, "decode matrix is singular");
    return FEC_OK;
}

// The pattern and id checks of the pattern-per-stripe calls (fec_decode_batch_mixed,
// fec_repair_batch), which need no GPU: the number of patterns, the call's own
// checks of them (check_each), then the ids.  Ids in host memory are checked
// here; ids in device memory (*idev >= 0) cannot be -- the kernels leave a
// stripe with an id >= npatterns unwritten.  pattern_of may be null (repair).
template <class F>
int check_patterns_and_ids(size_t npatterns, size_t nstripes, const unsigned* pattern_of, int* idev, F check_each) {
    if (npatterns == 0 && nstripes > 0)
        return set_status(FEC_EINVAL, "npatterns is 0: stripe 0 of %zu has no pattern", nstripes);
    if (npatterns > kMixedMaxPatterns)
        return set_status(FEC_EINVAL, "%zu patterns: a call takes at most %u", npatterns, unsigned(kMixedMaxPatterns));
    if (check_each()) return t_status;
    const int ngpu = gpu_available();
    *idev = ngpu && pattern_of ? pointer_device(pattern_of) : -1;
    if (pattern_of && *idev < 0)
        for (size_t s = 0; s < nstripes; ++s)
            if (pattern_of[s] >= npatterns)
                return set_status(FEC_EINVAL, "stripe %zu: pattern id %u out of range (npatterns = %zu)", s,
                                  pattern_of[s], npatterns);
    if (!ngpu) return set_status(FEC_ENODEV, "no GPU visible to HIP (the engine has no CPU path)");
    return FEC_OK;
}

// The k > kMixedMaxK fallback of those calls: maximal runs of consecutive
// stripes with one id.  Ids in device memory come to the host first; a run
// whose id names no pattern is skipped (device ids are not checked: such
// stripes stay unwritten, as on the kernels).  make(id, entry) builds the id's
// rows, once per call; apply(entry, s0, s1) runs stripes [s0, s1).
template <class Entry, class Make, class Apply>
int for_each_id_run(const unsigned* pattern_of, int idev, size_t nstripes, size_t npatterns, hipStream_t st, Make make,
                    Apply apply) {
    thread_local std::vector<unsigned> hids;
    const unsigned* ids = pattern_of;
    if (idev >= 0) {
        hipError_t e;
        hids.resize(nstripes);
        if ((e = hipMemcpyAsync(hids.data(), pattern_of, nstripes * sizeof(unsigned), hipMemcpyDeviceToHost, st)) !=
            hipSuccess)
            return hip_fail(e, "hipMemcpyAsync D2H (pattern_of)");
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
        ids = hids.data();
    }
    std::unordered_map<unsigned, Entry> cache;
    for (size_t s0 = 0; s0 < nstripes;) {
        size_t s1 = s0 + 1;
        while (s1 < nstripes && ids[s1] == ids[s0]) ++s1;
        if (ids[s0] < npatterns) {
            const auto ins = cache.try_emplace(ids[s0]);
            if (ins.second && make(ids[s0], ins.first->second)) return t_status;
            if (apply(ins.first->second, s0, s1)) return t_status;
        }
        s0 = s1;
    }
    return FEC_OK;
}

// Whether a pattern-per-stripe call of a wider code (4 < k <= 32) is ONE launch
// of the mix form of the bit-sliced kernels (kernels.hpp launch_bsr_mixed): r
// rows per pattern, blocks in device memory (page-locked host blocks keep the
// run path), the records within kBsrMixMaxBytes, ZFEC_HIP_MIXED_FUSED not 0.
bool fused_mixed_shape(unsigned k, size_t r, size_t sz, size_t npatterns, const BatchMem& mem) {
    return config().mixed_fused && mem.bdev[0] >= 0 && mem.bdev[1] >= 0 && r <= kRepairMaxRows &&
           bsr_mix_ok(k, static_cast<uint32_t>(r), sz) &&
           npatterns * bsr_mix_record_bytes(k, static_cast<uint32_t>(r)) <= kBsrMixMaxBytes;
}

int run_mixed(const fec_t* code, const gf* src, size_t sbs, size_t sss, gf* dst, size_t dbs, size_t dss,
              const unsigned* patterns, size_t npatterns, const unsigned* pattern_of, int idev, size_t sz,
              size_t nstripes, void* stream, unsigned flags) {
    const unsigned k = code->k;
    // device memory on one device, or page-locked host memory (read and written in place)
    const BatchBuf bufs[2] = {{src, (nstripes - 1) * sss + (k - 1) * sbs + sz, "src"},
                              {dst, (nstripes - 1) * dss + (k - 1) * dbs + sz, "dst"}};
    BatchMem mem;
    if (resolve_batch(mem, "fec_decode_batch_mixed", bufs, 2, "pattern_of", idev, stream, flags, kCaptureTables))
        return t_status;
    const gf* const zsrc = mem.z[0];
    gf* const zdst = const_cast<gf*>(mem.z[1]);
    hipStream_t st = mem.st;
    hipError_t e;
    // one launch: the register kernels for k <= 4, the mix form of the bit-sliced
    // kernels for wider codes on device memory (fused_mixed_shape)
    bool one = k <= kMixedMaxK || fused_mixed_shape(k, k, sz, npatterns, mem);
    if (one) {
        thread_local std::vector<uint8_t> rows;
        rows.resize(npatterns * k * k);
        for (size_t p = 0; p < npatterns; ++p)
            if (mixed_rows(code, patterns + p * k, &rows[p * k * k])) return t_status;
        const uint8_t* in[kMaxIn];
        uint8_t* out[kMaxIn];
        for (unsigned j = 0; j < k; ++j) {
            in[j] = zsrc + j * sbs;
            out[j] = zdst + j * dbs;
        }
        MixedSpec m;
        m.k = k;
        m.rows = rows.data();
        m.npatterns = static_cast<uint32_t>(npatterns);
        m.ids_host = idev < 0 ? pattern_of : nullptr;
        m.ids_dev = idev < 0 ? nullptr : pattern_of;
        m.in = in;
        m.out = out;
        m.sz = sz;
        m.nstripes = nstripes;
        m.in_sstride = sss;
        m.out_sstride = dss;
        ++t_launches;
        e = launch_mixed(m, st);
        if (e == hipErrorNotSupported && k > kMixedMaxK)
            one = false;  // the launch declined with nothing enqueued: the run path
        else if (e != hipSuccess)
            return hip_fail(e, "launch_mixed");
    }
    if (!one) {
        // what the one launch does not take: each run through the shared-pattern batched path
        const unsigned jf = (flags & FEC_FLAG_LIBRARY_STREAM) | FEC_FLAG_ASYNC;
        if (for_each_id_run<std::vector<uint8_t>>(
                pattern_of, idev, nstripes, npatterns, st,
                [&](unsigned id, std::vector<uint8_t>& rows) {
                    rows.resize(size_t(k) * k);
                    return mixed_rows(code, patterns + size_t(id) * k, rows.data());
                },
                [&](const std::vector<uint8_t>& rows, size_t s0, size_t s1) {
                    return run_batch(code, rows.data(), k, src + s0 * sss, sbs, sss, dst + s0 * dss, dbs, dss, sz,
                                     s1 - s0, stream, jf);
                }))
            return t_status;
    }
    if (!(flags & FEC_FLAG_ASYNC) && (e = hipStreamSynchronize(st)) != hipSuccess)
        return hip_fail(e, "hipStreamSynchronize");
    return set_status(FEC_OK);
}
}  // namespace

FEC_API int fec_mixed_decode_rows(const fec_t* code, const unsigned* pattern, gf* rows) {
    if (!valid_code(code)) return set_status(FEC_EINVAL, "invalid fec_t");
    if (!pattern) return set_status(FEC_EINVAL, "pattern is NULL");
    if (!rows) return set_status(FEC_EINVAL, "rows is NULL");
    if (check_pattern(code, pattern, 0)) return t_status;
    return guarded([&] {
        if (mixed_rows(code, pattern, rows)) return t_status;
        return set_status(FEC_OK);
    });
}

FEC_API int fec_decode_batch_mixed(const fec_t* code, const gf* src, size_t src_block_stride,
                                   size_t src_stripe_stride, gf* dst, size_t dst_block_stride,
                                   size_t dst_stripe_stride, const unsigned* patterns, size_t npatterns,
                                   const unsigned* pattern_of, size_t sz, size_t nstripes, void* stream,
                                   unsigned flags) {
    // every check that needs no GPU comes first
    if (!valid_code(code)) return set_status(FEC_EINVAL, "invalid fec_t");
    if (!src || !dst) return set_status(FEC_EINVAL, "NULL buffer");
    if (!patterns) return set_status(FEC_EINVAL, "patterns is NULL");
    if (!pattern_of) return set_status(FEC_EINVAL, "pattern_of is NULL");
    int idev = -1;
    if (check_patterns_and_ids(npatterns, nstripes, pattern_of, &idev, [&] {
            for (size_t p = 0; p < npatterns; ++p)
                if (check_pattern(code, patterns + p * code->k, p)) return t_status;
            return int(FEC_OK);
        }))
        return t_status;
    if (sz == 0 || nstripes == 0) return set_status(FEC_OK);
    return guarded([&] {
        return run_mixed(code, src, src_block_stride, src_stripe_stride, dst, dst_block_stride, dst_stripe_stride,
                         patterns, npatterns, pattern_of, idev, sz, nstripes, stream, flags);
    });
}

// ---- batched parity verification (scrub) ---------------------------------------------
namespace {
// nb block numbers of a verify call: k + 1 <= nb <= n, each < n, all distinct.
int check_verify_nums(const fec_t* code, const unsigned* nums, size_t nb) {
    if (nb <= code->k)
        return set_status(FEC_EINVAL, "nothing to check: %zu blocks per stripe, a check needs more than k = %u", nb,
                          unsigned(code->k));
    if (nb > code->n)
        return set_status(FEC_EINVAL, "%zu blocks per stripe, but the code has only n = %u", nb, unsigned(code->n));
    for (size_t j = 0; j < nb; ++j)
        if (nums[j] >= code->n)
            return set_status(FEC_EINVAL, "block number %u out of range (n = %u)", nums[j], unsigned(code->n));
    unsigned char seen[256] = {};
    for (size_t j = 0; j < nb; ++j) {
        if (seen[nums[j]]) return set_status(FEC_EINVAL, "duplicate block number %u", nums[j]);
        seen[nums[j]] = 1;
    }
    return FEC_OK;
}

// The argument checks of the verify / locate / correct family, none of which
// needs a GPU.  A *_batch call names its block buffer (`blocks`, "src" or
// "blocks") and needs a GPU in the end; a *_rows call passes blocks_name null.
// `out` is the call's result pointer (rows, mismatch, culprit).
int check_verify_call(const fec_t* code, const void* blocks, const char* blocks_name, const unsigned* nums, size_t nb,
                      const void* out, const char* out_name) {
    if (!valid_code(code)) return set_status(FEC_EINVAL, "invalid fec_t");
    if (blocks_name && !blocks) return set_status(FEC_EINVAL, "NULL buffer: %s", blocks_name);
    if (!nums) return set_status(FEC_EINVAL, "block_nums is NULL");
    if (!out) return set_status(FEC_EINVAL, "%s is NULL", out_name);
    if (check_verify_nums(code, nums, nb)) return t_status;
    if (blocks_name && !gpu_available())
        return set_status(FEC_ENODEV, "no GPU visible to HIP (the engine has no CPU path)");
    return FEC_OK;
}

// out[0..k) = row `num` of enc_matrix times the k x k matrix inv: the row that
// yields block `num` from the slots inv decodes (fec_verify_rows, fec_repair_rows).
void enc_row_times(const fec_t* code, unsigned num, const uint8_t* inv, uint8_t* out) {
    const unsigned k = code->k;
    const uint8_t* e = code->enc_matrix + size_t(num) * k;
    for (unsigned j = 0; j < k; ++j) {
        uint8_t acc = 0;
        for (unsigned l = 0; l < k; ++l) acc ^= gf_mul(e[l], inv[size_t(l) * k + j]);
        out[j] = acc;
    }
}

// P = E[checks] . inverse(E[basis]), c x k row-major: row i yields the block in
// slot k + i from the k basis slots.
int verify_rows(const fec_t* code, const unsigned* nums, size_t nb, uint8_t* P) {
    const unsigned k = code->k;
    thread_local std::vector<uint8_t> inv;
    inv.resize(size_t(k) * k);
    if (mixed_rows(code, nums, inv.data())) return t_status;
    for (size_t i = 0; i + k < nb; ++i) enc_row_times(code, nums[k + i], inv.data(), P + i * k);
    return FEC_OK;
}

// Device memory of at least `bytes` the thread keeps per device.  Growing it
// first waits for the last verify call that used the old one.
int ensure_verify_buf(DevCtx& d, void*& buf, size_t& cap, size_t bytes) {
    if (bytes <= cap) return FEC_OK;
    if (d.verify_busy) (void)hipEventSynchronize(d.ev_verify);
    if (buf) (void)hipFree(buf);
    buf = nullptr;
    cap = 0;
    const size_t want = align_up(std::max<size_t>(bytes, size_t(1) << 20), 4096);
    const hipError_t e = hipMalloc(&buf, want);
    if (e != hipSuccess) return set_status(FEC_ENOMEM, "hipMalloc(%zu): %s", want, hipGetErrorString(e));
    cap = want;
    return FEC_OK;
}

// The blocks and words of a verify / locate call, as the kernels see them.
struct VerifyArgs {
    const uint8_t* P;  // c x k
    unsigned k, c;
    const gf* src;
    size_t sbs, sss, sz, nstripes;
    uint32_t* mask;
    unsigned words;
    hipStream_t st;
};

// The c check rows against the k basis blocks in launches of at most `rows`
// rows, the bit index advancing: launch(spec, stream), named `what` in a
// failure's message.  declined (may be null): a launch may find no kernel on
// this device (hipErrorNotSupported); *declined is set, whatever earlier
// launches OR-ed in stays valid, and the caller runs the two-step path.
template <class Launch>
int verify_groups(const VerifyArgs& a, unsigned rows, Launch launch, const char* what, bool* declined = nullptr) {
    const uint8_t* in[kMaxIn];
    const uint8_t* chk[kVerifyBsrRows];
    for (unsigned j = 0; j < a.k; ++j) in[j] = a.src + j * a.sbs;
    for (unsigned g0 = 0; g0 < a.c; g0 += rows) {
        const unsigned rg = std::min(rows, a.c - g0);
        for (unsigned i = 0; i < rg; ++i) chk[i] = a.src + size_t(a.k + g0 + i) * a.sbs;
        VerifySpec v;
        v.coef = a.P + size_t(g0) * a.k;
        v.coef_stride = a.k;
        v.k = a.k;
        v.r = rg;
        v.in = in;
        v.chk = chk;
        v.sz = a.sz;
        v.nstripes = a.nstripes;
        v.sstride = a.sss;
        v.mismatch = a.mask;
        v.words = a.words;
        v.bit0 = g0;
        const hipError_t e = launch(v, a.st);
        if (declined && e == hipErrorNotSupported) {
            (void)hipGetLastError();
            *declined = true;
            return FEC_OK;
        }
        ++t_launches;  // every launch made, failed or not
        if (e != hipSuccess) return hip_fail(e, what);
    }
    return FEC_OK;
}

// Every other shape: the expected check rows into scratch through
// apply_matrix (whatever kernel it picks), then rows_differ against the stored
// rows.  The scratch holds c rows of `pitch` bytes per stripe and at most
// Config::verify_scratch bytes: a batch goes in runs of stripes that fit, a
// stripe larger than that in byte ranges.  The bits OR together, so the
// cutting is invisible.  With `loc` (fec_locate_batch) rows_locate takes the
// place of rows_differ: it also reads row 0's pair and ORs excluded bits from
// bit loc->xbit on, against the Q tables at loc->qtab.
struct LocateRows {
    const uint32_t* qtab;  // device memory
    unsigned xbit;
};
int verify_scratch_path(DevCtx& d, const VerifyArgs& a, const LocateRows* loc = nullptr) {
    const auto [P, k, c, src, sbs, sss, sz, nstripes, mask, words, st] = a;
    const size_t cap = config().verify_scratch;
    size_t len = sz, run = 1;
    if (size_t(c) * align_up(sz, 128) <= cap)
        run = std::min(nstripes, cap / (size_t(c) * align_up(sz, 128)));
    else
        len = cap / c / 128 * 128;
    const size_t pitch = align_up(len, 128), sstride = size_t(c) * pitch;
    if (ensure_verify_buf(d, d.vbuf, d.vcap, run * sstride)) return t_status;
    uint8_t* const scratch = static_cast<uint8_t*>(d.vbuf);
    const uint8_t* in[kMaxWideIn];
    uint8_t* out[kMaxWideIn];
    const uint8_t* stored[kMaxOut];
    for (unsigned i = 0; i < c; ++i) out[i] = scratch + i * pitch;
    for (size_t s0 = 0; s0 < nstripes; s0 += run) {
        const size_t ns = std::min(run, nstripes - s0);
        for (size_t b0 = 0; b0 < sz; b0 += len) {
            const size_t l = std::min(len, sz - b0);
            const gf* base = src + s0 * sss + b0;
            for (unsigned j = 0; j < k; ++j) in[j] = base + j * sbs;
            if (apply_matrix(P, k, c, in, out, l, ns, sss, sstride, st)) return t_status;
            for (unsigned g0 = 0; g0 < c; g0 += kMaxOut) {
                const unsigned rg = std::min<unsigned>(kMaxOut, c - g0);
                for (unsigned i = 0; i < rg; ++i) stored[i] = base + size_t(k + g0 + i) * sbs;
                DifferSpec f;
                f.r = rg;
                f.a = out + g0;
                f.b = stored;
                f.sz = l;
                f.nstripes = ns;
                f.a_sstride = sstride;
                f.b_sstride = sss;
                f.mismatch = mask + s0 * words;
                f.words = words;
                f.bit0 = g0;
                ++t_launches;
                if (loc) {
                    const hipError_t e =
                        launch_rows_locate(f, out[0], base + size_t(k) * sbs, k, loc->xbit, loc->qtab, st);
                    if (e != hipSuccess) return hip_fail(e, "launch_rows_locate");
                    continue;
                }
                const hipError_t e = launch_rows_differ(f, st);
                if (e != hipSuccess) return hip_fail(e, "launch_rows_differ");
            }
        }
    }
    return FEC_OK;
}

// 4 < k <= 32 on device memory, from Config::verify_fused_min 2-KiB units up:
// matverify_bsr computes the check rows as bit-planes in registers and
// compares them with the stored rows in the same launch -- k + c rows read, no
// scratch, so no cutting into runs and no buffer shared between streams.  More
// than kVerifyBsrRows checks run as launches of at most that many, the bit
// index advancing (the basis is re-read per launch: still fewer bytes than the
// two-step path's k + 3c).  Every launch must have a shape the kernels take,
// or the whole call keeps the two-step path.
bool verify_fused_ok(unsigned k, unsigned c, size_t sz, size_t nstripes) {
    if (k <= 4 || sz < 2048) return false;
    for (unsigned g0 = 0; g0 < c; g0 += kVerifyBsrRows)
        if (!verify_bsr_ok(k, std::min(kVerifyBsrRows, c - g0), sz)) return false;
    const uint64_t units = uint64_t((sz + 2047) / 2048) * nstripes;
    return units >= config().verify_fused_min && units < (1ull << 32) - (1ull << 24);
}

// The order of the thread's shared verify buffers (vbuf, vmask) among calls on
// any streams.  acquire(): `st` waits, on the GPU, for the call that used them
// last.  release(), once this call has enqueued all it will: whatever was
// enqueued uses the buffers, so they stay busy whatever happened; it does
// nothing for a call that never acquired them.
struct VerifyOrder {
    DevCtx& d;
    hipStream_t st;
    bool held = false;
    int init() {
        hipError_t e;
        if (!d.ev_verify && (e = hipEventCreateWithFlags(&d.ev_verify, hipEventDisableTiming)) != hipSuccess)
            return hip_fail(e, "hipEventCreateWithFlags");
        return FEC_OK;
    }
    int acquire() {
        hipError_t e;
        if (held) return FEC_OK;
        held = true;
        if (d.verify_busy && (e = hipStreamWaitEvent(st, d.ev_verify, 0)) != hipSuccess)
            return hip_fail(e, "hipStreamWaitEvent");
        return FEC_OK;
    }
    void release() {
        if (!held) return;
        if (hipEventRecord(d.ev_verify, st) == hipSuccess)
            d.verify_busy = true;
        else
            (void)hipStreamSynchronize(st);
    }
};

int run_verify(const fec_t* code, const gf* src, size_t sbs, size_t sss, const unsigned* nums, size_t nb, size_t sz,
               size_t nstripes, unsigned* mismatch, void* stream, unsigned flags) {
    const unsigned k = code->k, c = static_cast<unsigned>(nb - k), words = (c + 31) / 32;
    if (nstripes >= (size_t(1) << 32)) return set_status(FEC_EINVAL, "%zu stripes: a call takes fewer than 2^32", nstripes);
    const size_t mask_bytes = nstripes * words * sizeof(uint32_t);
    const int mdev = pointer_device(mismatch);
    // device memory on one device, or page-locked host memory (read in place); sz == 0 reads no block
    const BatchBuf buf = {src, (nstripes - 1) * sss + (nb - 1) * sbs + sz, "src"};
    BatchMem mem;
    if (resolve_batch(mem, "fec_verify_batch", &buf, sz ? 1 : 0, "mismatch", mdev, stream, flags, kCaptureMemory))
        return t_status;
    DevCtx* const d = mem.d;
    hipStream_t st = mem.st;
    hipError_t e;
    VerifyOrder order{*d, st};
    if (order.init()) return t_status;
    // the thread's scratch and mask buffer: wait (on the GPU) for the call that used them last
    // (the fused kernels read page-locked host blocks no better than the two
    // steps do -- both move k + c over PCIe -- so those keep the two-step path)
    const bool reg = k <= 4, fused = !reg && sz && mem.bdev[0] >= 0 && verify_fused_ok(k, c, sz, nstripes);
    if ((mdev < 0 || (!reg && !fused && sz)) && order.acquire()) return t_status;
    // mismatch in host memory: the kernels' device-scope atomics must not aim
    // at host memory over PCIe, so the words are gathered in device memory
    if (mdev < 0 && ensure_verify_buf(*d, d->vmask, d->vmask_cap, mask_bytes)) return t_status;
    uint32_t* const mask = mdev < 0 ? static_cast<uint32_t*>(d->vmask) : mismatch;
    if ((e = hipMemsetAsync(mask, 0, mask_bytes, st)) != hipSuccess) return hip_fail(e, "hipMemsetAsync (mismatch)");
    int rc = FEC_OK;
    if (sz) {
        thread_local std::vector<uint8_t> P;
        P.resize(size_t(c) * k);
        rc = verify_rows(code, nums, nb, P.data());
        const VerifyArgs a = {P.data(), k, c, mem.z[0], sbs, sss, sz, nstripes, mask, words, st};
        bool two_step = !reg && !fused;
        if (!rc && fused) {
            rc = verify_groups(a, kVerifyBsrRows, launch_verify_bsr, "launch_verify_bsr", &two_step);
            // declined: the scratch after all, ordered after its last user
            if (!rc && two_step) rc = order.acquire();
        }
        if (!rc && reg) rc = verify_groups(a, 8, launch_verify, "launch_verify");  // matverify_reg
        if (!rc && two_step) rc = verify_scratch_path(*d, a);
    }
    if (!rc && mdev < 0 && (e = hipMemcpyAsync(mismatch, mask, mask_bytes, hipMemcpyDeviceToHost, st)) != hipSuccess)
        rc = hip_fail(e, "hipMemcpyAsync D2H (mismatch)");
    order.release();
    if (rc) return rc;
    if ((mdev < 0 || !(flags & FEC_FLAG_ASYNC)) && (e = hipStreamSynchronize(st)) != hipSuccess)
        return hip_fail(e, "hipStreamSynchronize");
    return set_status(FEC_OK);
}
}  // namespace

FEC_API int fec_verify_rows(const fec_t* code, const unsigned* block_nums, size_t num_block_nums, gf* rows) {
    if (check_verify_call(code, nullptr, nullptr, block_nums, num_block_nums, rows, "rows")) return t_status;
    return guarded([&] {
        if (verify_rows(code, block_nums, num_block_nums, rows)) return t_status;
        return set_status(FEC_OK);
    });
}

FEC_API int fec_verify_batch(const fec_t* code, const gf* src, size_t src_block_stride, size_t src_stripe_stride,
                             const unsigned* block_nums, size_t num_block_nums, size_t sz, size_t nstripes,
                             unsigned* mismatch, void* stream, unsigned flags) {
    // every check that needs no GPU comes first
    if (check_verify_call(code, src, "src", block_nums, num_block_nums, mismatch, "mismatch")) return t_status;
    if (nstripes == 0) return set_status(FEC_OK);
    return guarded([&] {
        return run_verify(code, src, src_block_stride, src_stripe_stride, block_nums, num_block_nums, sz, nstripes,
                          mismatch, stream, flags);
    });
}

// ---- batched single-block error location ---------------------------------------------------
namespace {
// Q[i][j] = P[i][j] / P[0][j] for i = 1..c-1, (c-1) x k row-major: the ratios a
// single corrupt basis slot j imposes on the syndromes.  P has no zero entry
// (the held blocks form an MDS code).
void locate_rows(const uint8_t* P, unsigned k, unsigned c, uint8_t* Q) {
    const Field& f = field();
    for (unsigned i = 1; i < c; ++i)
        for (unsigned j = 0; j < k; ++j) Q[size_t(i - 1) * k + j] = f.mul[P[size_t(i) * k + j]][f.inv[P[j]]];
}

// The nb x k correction matrix (fec_correct_rows): row h rebuilds slot h from
// slots 0..k-1, slot k (check 0) standing in for slot h when h < k.  Solving
// check 0's equation c_0 = sum_l P[0][l] . b_l for b_h gives R[l] = P[0][l] /
// P[0][h] for l != h and R[h] = 1 / P[0][h] (applied to c_0); rows k.. are P.
void correct_rows(const uint8_t* P, unsigned k, unsigned c, uint8_t* R) {
    const Field& f = field();
    for (unsigned h = 0; h < k; ++h) {
        const uint8_t ih = f.inv[P[h]];
        for (unsigned l = 0; l < k; ++l) R[size_t(h) * k + l] = l == h ? ih : f.mul[P[l]][ih];
    }
    std::memcpy(R + size_t(k) * k, P, size_t(c) * k);
}

// Column h of the c x nb matrix [P | I] at row i.
inline uint8_t column_at(const uint8_t* P, unsigned k, unsigned h, unsigned i) {
    return h < k ? P[size_t(i) * k + h] : uint8_t(h - k == i);
}

// The pivot form of a (c-2) x c matrix N of rank c - 2 with N . p_a = N . p_b = 0
// (fec_locate2_rows), c >= 3: out[0..1] = two rows r0, r1 on which [p_a p_b] has
// a nonzero minor -- r0 the first row where p_a is nonzero, r1 the first other
// row that completes one; p_a and p_b are independent, so it exists -- then
// for every other row i, ascending, (i, alpha, beta) with
//     p_h[i] = alpha . p_h[r0] + beta . p_h[r1]   for h = a and h = b
// (a 2 x 2 solve), i.e. row e_i + alpha . e_r0 + beta . e_r1 of N.  O(c) per pair.
// False (nothing usable written) if no such rows exist, which an MDS code rules out.
bool pair_pivots(const uint8_t* P, unsigned k, unsigned c, unsigned a, unsigned b, uint8_t* out) {
    const Field& f = field();
    unsigned r0 = 0, r1 = 0;
    while (r0 < c && !column_at(P, k, a, r0)) ++r0;
    if (r0 == c) return false;
    const uint8_t a0 = column_at(P, k, a, r0), b0 = column_at(P, k, b, r0);
    uint8_t a1 = 0, b1 = 0, det = 0;
    for (; r1 < c; ++r1) {
        if (r1 == r0) continue;
        a1 = column_at(P, k, a, r1);
        b1 = column_at(P, k, b, r1);
        det = f.mul[a0][b1] ^ f.mul[a1][b0];
        if (det) break;
    }
    if (r1 == c) return false;
    const uint8_t id = f.inv[det];
    out[0] = uint8_t(r0);
    out[1] = uint8_t(r1);
    out += 2;
    for (unsigned i = 0; i < c; ++i) {
        if (i == r0 || i == r1) continue;
        const uint8_t ai = column_at(P, k, a, i), bi = column_at(P, k, b, i);
        out[0] = uint8_t(i);
        out[1] = f.mul[f.mul[b1][ai] ^ f.mul[a1][bi]][id];
        out[2] = f.mul[f.mul[b0][ai] ^ f.mul[a0][bi]][id];
        out += 3;
    }
    return true;
}

// fec_correct2_rows, c >= 2: the k lowest slots outside {a, b}, ascending, into
// sources, and the 2 x k rows that yield slots a and b from them, by solving
// the first check equations not lost for the lost basis slots (O(k) per pair):
//   both checks:     the basis; rows P[a-k] and P[b-k];
//   a basis, b check: check q (the first that is not b) solved for slot a, then
//                     check b's row with that substituted for slot a;
//   both basis:       checks 0 and 1 solved for slots a and b (a 2 x 2 solve).
void pair_correct_rows(const uint8_t* P, unsigned k, unsigned a, unsigned b, uint32_t* sources, uint8_t* rows) {
    const Field& f = field();
    uint8_t* const ra = rows;
    uint8_t* const rb = rows + k;
    if (a >= k) {
        for (unsigned l = 0; l < k; ++l) sources[l] = l;
        std::memcpy(ra, P + size_t(a - k) * k, k);
        std::memcpy(rb, P + size_t(b - k) * k, k);
        return;
    }
    unsigned n = 0;
    if (b >= k) {
        const unsigned q = b == k ? 1 : 0;
        const uint8_t* const pq = P + size_t(q) * k;
        const uint8_t* const pb = P + size_t(b - k) * k;
        const uint8_t ia = f.inv[pq[a]];
        for (unsigned l = 0; l < k; ++l) {
            if (l == a) continue;
            sources[n] = l;
            ra[n] = f.mul[pq[l]][ia];
            rb[n] = pb[l] ^ f.mul[pb[a]][ra[n]];
            ++n;
        }
        sources[n] = k + q;
        ra[n] = ia;
        rb[n] = f.mul[pb[a]][ia];
        return;
    }
    const uint8_t* const p0 = P;
    const uint8_t* const p1 = P + k;
    const uint8_t id = f.inv[f.mul[p0[a]][p1[b]] ^ f.mul[p0[b]][p1[a]]];
    for (unsigned l = 0; l < k; ++l) {
        if (l == a || l == b) continue;
        sources[n] = l;
        ra[n] = f.mul[f.mul[p1[b]][p0[l]] ^ f.mul[p0[b]][p1[l]]][id];
        rb[n] = f.mul[f.mul[p1[a]][p0[l]] ^ f.mul[p0[a]][p1[l]]][id];
        ++n;
    }
    sources[n] = k;
    sources[n + 1] = k + 1;
    ra[n] = f.mul[p1[b]][id];
    ra[n + 1] = f.mul[p0[b]][id];
    rb[n] = f.mul[p1[a]][id];
    rb[n + 1] = f.mul[p0[a]][id];
}

// The records of a pair pass, for launch_pairs and launch_pairs_ragged: every
// pair's pivots (pair_pivots) and, with heal, its sources and rows
// (pair_correct_rows), in pair-index order.  The vectors are the thread's.
struct PairRecs {
    const uint8_t* pivots = nullptr;
    const uint32_t* sources = nullptr;  // null: locate only
    const uint8_t* crows = nullptr;
    int build(const uint8_t* P, unsigned k, unsigned c, bool heal, const char* fn) {
        const unsigned nb = k + c, npairs = nb * (nb - 1) / 2;
        const size_t pbytes = 2 + 3 * size_t(c - 2);
        thread_local std::vector<uint8_t> pv, cr;
        thread_local std::vector<uint32_t> so;
        pv.resize(npairs * pbytes);
        if (heal) {
            so.resize(size_t(npairs) * k);
            cr.resize(size_t(npairs) * 2 * k);
        }
        unsigned p = 0;
        for (unsigned a = 0; a + 1 < nb; ++a)
            for (unsigned b = a + 1; b < nb; ++b, ++p) {
                if (!pair_pivots(P, k, c, a, b, pv.data() + p * pbytes))
                    return set_status(FEC_ESINGULAR, "%s: slots %u and %u have dependent check columns", fn, a, b);
                if (heal) pair_correct_rows(P, k, a, b, so.data() + size_t(p) * k, cr.data() + size_t(p) * 2 * k);
            }
        pivots = pv.data();
        sources = heal ? so.data() : nullptr;
        crows = heal ? cr.data() : nullptr;
        return FEC_OK;
    }
};

// The working words of a call (W = ceil(c/32) + ceil(k/32) per stripe, mismatch
// bits from bit 0, excluded bits from bit 32*ceil(c/32)) live in the thread's
// vmask buffer, under run_verify's ev_verify ordering; a host-side culprit is
// gathered behind them.
//
// With `heal` (fec_correct_batch; `fn` names the call in messages) one
// correction follows locate_finish in the same stream, over the verdict words
// in device memory: the host never sees them.
//
// `plane` (pairs): the words from culprit's plane 0 to its plane 1, 0 for
// nstripes.  A run of a ragged call passes the whole call's stripe count and
// culprit + s0, so its words land in the whole call's planes; words gathered
// for a host-side culprit stay nstripes apart and are copied back per plane.
int run_locate(const fec_t* code, const gf* src, size_t sbs, size_t sss, const unsigned* nums, size_t nb, size_t sz,
               size_t nstripes, unsigned* culprit, void* stream, unsigned flags, const char* fn = "fec_locate_batch",
               bool heal = false, bool pairs = false, size_t plane = 0) {
    const unsigned k = code->k, c = static_cast<unsigned>(nb - k), cw = (c + 31) / 32, words = cw + (k + 31) / 32;
    const unsigned xbit = 32 * cw;
    if (nstripes >= (size_t(1) << 32)) return set_status(FEC_EINVAL, "%zu stripes: a call takes fewer than 2^32", nstripes);
    // fec_locate2_batch / fec_correct2_batch: two verdict planes, and where the pair pass runs the dirty
    // list (its counter first, cleared with the working words) and the entries' pair words behind the bits
    const bool pass2 = pairs && sz && pairs_shape_ok(k, c);
    const size_t pw = pass2 ? pairs_words(static_cast<uint32_t>(nb)) : 0;
    const size_t work_bytes = nstripes * words * sizeof(uint32_t);
    const size_t out_bytes = nstripes * sizeof(uint32_t) * (pairs ? 2 : 1);
    const size_t pair_words = pass2 ? 1 + nstripes + nstripes * pw : 0;
    const int cdev = pointer_device(culprit);
    const size_t oplane = cdev >= 0 && plane ? plane : nstripes;  // of the words the kernels write
    // device memory on one device, or page-locked host memory (read in place); sz == 0 reads no block
    const BatchBuf buf = {src, (nstripes - 1) * sss + (nb - 1) * sbs + sz, heal ? "blocks" : "src"};
    BatchMem mem;
    if (resolve_batch(mem, fn, &buf, sz ? 1 : 0, "culprit", cdev, stream, flags, kCaptureMemory)) return t_status;
    DevCtx* const d = mem.d;
    const gf* const zsrc = mem.z[0];
    hipStream_t st = mem.st;
    hipError_t e;
    // the thread's working words (and scratch): wait (on the GPU) for the call that used them last
    VerifyOrder order{*d, st};
    if (order.init() || order.acquire()) return t_status;
    if (ensure_verify_buf(*d, d->vmask, d->vmask_cap,
                          work_bytes + pair_words * sizeof(uint32_t) + (cdev < 0 ? out_bytes : 0)))
        return t_status;
    uint32_t* const bits = static_cast<uint32_t*>(d->vmask);
    uint32_t* const list = pass2 ? bits + nstripes * words : nullptr;
    uint32_t* const pairbits = pass2 ? list + 1 + nstripes : nullptr;
    uint32_t* const out = cdev < 0 ? bits + nstripes * words + pair_words : culprit;
    if ((e = hipMemsetAsync(bits, 0, work_bytes + (pass2 ? sizeof(uint32_t) : 0), st)) != hipSuccess)
        return hip_fail(e, "hipMemsetAsync (working words)");
    int rc = FEC_OK;
    thread_local std::vector<uint8_t> P, Q, R;
    if (sz) {
        P.resize(size_t(c) * k);
        Q.resize(size_t(c - 1) * k);
        rc = verify_rows(code, nums, nb, P.data());
        const VerifyArgs a = {P.data(), k, c, zsrc, sbs, sss, sz, nstripes, bits, words, st};
        if (!rc && c == 1) {
            // one check cannot tell: the verify kernels' bit, then UNKNOWN
            rc = k <= 4 ? verify_groups(a, 8, launch_verify, "launch_verify") : verify_scratch_path(*d, a);
        } else if (!rc && k <= 4 && c <= 8) {
            // matlocate_reg: all c checks in one launch
            locate_rows(P.data(), k, c, Q.data());
            rc = verify_groups(
                a, 8, [&](const VerifySpec& v, hipStream_t s) { return launch_locate(v, Q.data(), xbit, s); },
                "launch_locate");
        } else if (!rc) {
            locate_rows(P.data(), k, c, Q.data());
            LocateTables tabs;
            if ((e = locate_tables_upload(Q.data(), k, c, st, &tabs)) != hipSuccess) {
                rc = hip_fail(e, "locate_tables_upload");
            } else {
                const LocateRows loc{tabs.dev, xbit};
                rc = verify_scratch_path(*d, a, &loc);
                locate_tables_release(tabs, st);
            }
        }
    }
    if (!rc) {
        // the block-reading kernel stays fec_last_kernel_name()'s answer
        ++t_launches;
        if (pairs) {
            if ((e = launch_locate2_finish(bits, words, k, c, nstripes, out, list, pairbits, st, oplane)) !=
                hipSuccess)
                rc = hip_fail(e, "launch_locate2_finish");
        } else if ((e = launch_locate_finish(bits, words, k, c, nstripes, out, st)) != hipSuccess) {
            rc = hip_fail(e, "launch_locate_finish");
        }
    }
    if (!rc && heal && sz) {
        // row h of the nb x k correction matrix rebuilds slot h (zsrc is the caller's writable blocks)
        R.resize(nb * k);
        correct_rows(P.data(), k, c, R.data());
        CorrectSpec cs;
        cs.k = k;
        cs.nb = static_cast<uint32_t>(nb);
        cs.rows = R.data();
        cs.blocks = const_cast<uint8_t*>(zsrc);
        cs.bstride = sbs;
        cs.sstride = sss;
        cs.sz = sz;
        cs.nstripes = nstripes;
        cs.verdict = out;
        ++t_launches;
        if ((e = launch_correct(cs, st)) != hipSuccess) rc = hip_fail(e, "launch_correct");
    }
    if (!rc && pass2) {
        // plane 0 still reads MANY for the listed stripes: the pair pass names (a, b) and, with heal, rewrites them
        PairRecs recs;
        rc = recs.build(P.data(), k, c, heal, fn);
        PairsSpec ps;
        ps.k = k;
        ps.c = c;
        ps.P = P.data();
        ps.pivots = recs.pivots;
        ps.sources = recs.sources;
        ps.crows = recs.crows;
        ps.plane = oplane;
        ps.blocks = const_cast<uint8_t*>(zsrc);
        ps.bstride = sbs;
        ps.sstride = sss;
        ps.sz = sz;
        ps.nstripes = nstripes;
        ps.list = list;
        ps.pairbits = pairbits;
        ps.culprit = out;
        if (!rc) {
            t_launches += heal ? 3 : 2;
            if ((e = launch_pairs(ps, st)) != hipSuccess) rc = hip_fail(e, "launch_pairs");
        }
    }
    if (!rc && cdev < 0) {
        // (the caller's planes lie further apart than the gathered ones: one copy per plane)
        const bool split = pairs && plane && plane != nstripes;
        if ((e = hipMemcpyAsync(culprit, out, split ? out_bytes / 2 : out_bytes, hipMemcpyDeviceToHost, st)) !=
                hipSuccess ||
            (split && (e = hipMemcpyAsync(culprit + plane, out + nstripes, out_bytes / 2, hipMemcpyDeviceToHost,
                                          st)) != hipSuccess))
            rc = hip_fail(e, "hipMemcpyAsync D2H (culprit)");
    }
    order.release();
    if (rc) return rc;
    if ((cdev < 0 || !(flags & FEC_FLAG_ASYNC)) && (e = hipStreamSynchronize(st)) != hipSuccess)
        return hip_fail(e, "hipStreamSynchronize");
    return set_status(FEC_OK);
}

// fec_locate_rows / fec_correct_rows: `derive` (locate_rows, correct_rows) of the block numbers' P.
int rows_from_P(const fec_t* code, const unsigned* block_nums, size_t num_block_nums, gf* rows,
                void (*derive)(const uint8_t*, unsigned, unsigned, uint8_t*)) {
    if (check_verify_call(code, nullptr, nullptr, block_nums, num_block_nums, rows, "rows")) return t_status;
    return guarded([&] {
        const unsigned k = code->k, c = static_cast<unsigned>(num_block_nums - k);
        thread_local std::vector<uint8_t> P;
        P.resize(size_t(c) * k);
        if (verify_rows(code, block_nums, num_block_nums, P.data())) return t_status;
        derive(P.data(), k, c, rows);
        return set_status(FEC_OK);
    });
}
}  // namespace

FEC_API int fec_locate_rows(const fec_t* code, const unsigned* block_nums, size_t num_block_nums, gf* rows) {
    return rows_from_P(code, block_nums, num_block_nums, rows, locate_rows);
}

FEC_API int fec_locate_batch(const fec_t* code, const gf* src, size_t src_block_stride, size_t src_stripe_stride,
                             const unsigned* block_nums, size_t num_block_nums, size_t sz, size_t nstripes,
                             unsigned* culprit, void* stream, unsigned flags) {
    // every check that needs no GPU comes first
    if (check_verify_call(code, src, "src", block_nums, num_block_nums, culprit, "culprit")) return t_status;
    if (nstripes == 0) return set_status(FEC_OK);
    return guarded([&] {
        return run_locate(code, src, src_block_stride, src_stripe_stride, block_nums, num_block_nums, sz, nstripes,
                          culprit, stream, flags);
    });
}

// ---- ragged scrub: verify and locate, a size per stripe --------------------------------------
namespace {
struct ScrubCall {
    const char* fn;
    bool locate;
    const gf* src;
    size_t src_bytes, sbs;
    const unsigned long long* soff;
    const unsigned long long* sizes;
    const unsigned* nums;
    size_t nb, nstripes;
    unsigned* out;  // mismatch or culprit
    void* stream;
    unsigned flags;
    bool heal = false;   // fec_correct_batch_ragged: src is the caller's writable blocks
    bool pairs = false;  // fec_locate2_batch_ragged / fec_correct2_batch_ragged: out is two planes of nstripes words
    const char* arena() const { return heal ? "blocks" : "src"; }
};

RaggedArgs ragged_args(const ScrubCall& c) {
    return RaggedArgs{c.fn,
                      c.heal ? "%s: sizes and offsets are of mixed memory kinds: both in host memory, or both in device "
                               "memory on the blocks' device"
                             : "%s: sizes and src_offsets are of mixed memory kinds: both in host memory, or both in "
                               "device memory on the blocks' device",
                      1, {{c.arena(), c.heal ? "offsets" : "src_offsets", c.heal ? "bytes" : "src_bytes",
                                 c.src_bytes, c.sbs, c.nb}, {}},
                      c.nstripes, c.sizes, {c.soff, nullptr}};
}

// Every check of a ragged scrub call that needs no GPU, in the header's order.
// *ddev: the descriptor arrays' device, -1 host memory.
int check_ragged_scrub(const fec_t* code, const ScrubCall& c, int* ddev) {
    if (!valid_code(code)) return set_status(FEC_EINVAL, "%s: invalid fec_t", c.fn);
    const struct {
        const void* p;
        const char* name;
    } args[] = {{c.src, c.arena()},
                {c.sizes, "sizes"},
                {c.soff, ragged_args(c).a[0].off_name},
                {c.nums, "block_nums"},
                {c.out, c.locate ? "culprit" : "mismatch"}};
    for (const auto& a : args)
        if (!a.p) return set_status(FEC_EINVAL, "%s: %s is NULL", c.fn, a.name);
    if (check_verify_nums(code, c.nums, c.nb)) {
        const std::string msg = t_msg;  // fec_verify_batch's checks, named as this call's
        return set_status(t_status, "%s: %s", c.fn, msg.c_str());
    }
    return check_ragged(ragged_args(c), ddev);
}

// k <= 4 (a location: c <= 8): matverify_ragged / matlocate_ragged.  The
// working words of a location, and a host-side result gathered behind them,
// live in the thread's vmask buffer under run_verify's ev_verify ordering.
int run_ragged_scrub_fused(const fec_t* code, const ScrubCall& c, int ddev, int rdev, BatchMem& mem) {
    const unsigned k = code->k, cc = static_cast<unsigned>(c.nb - k), cw = (cc + 31) / 32;
    const unsigned words = c.locate ? cw + (k + 31) / 32 : cw, xbit = 32 * cw;
    const size_t ns = c.nstripes;
    // the pair pass (c.pairs implies c.locate): the dirty list, its counter first and cleared with the
    // working words, and the entries' pair words lie behind the working words, as in run_locate
    const bool pass2 = c.pairs && pairs_shape_ok(k, cc);
    const size_t pw = pass2 ? pairs_words(static_cast<uint32_t>(c.nb)) : 0;
    const size_t pair_words = pass2 ? 1 + ns + ns * pw : 0;
    const size_t work_bytes = ns * words * sizeof(uint32_t);
    const size_t out_bytes = ns * (c.pairs ? 2 : c.locate ? 1 : cw) * sizeof(uint32_t);
    DevCtx* const d = mem.d;
    hipStream_t st = mem.st;
    hipError_t e;
    VerifyOrder order{*d, st};
    if (order.init()) return t_status;
    const bool own = c.locate || rdev < 0;  // words the library owns are in use
    if (own) {
        if (order.acquire()) return t_status;
        if (ensure_verify_buf(*d, d->vmask, d->vmask_cap,
                              (c.locate ? work_bytes + pair_words * sizeof(uint32_t) : 0) +
                                  (rdev < 0 ? out_bytes : 0)))
            return t_status;
    }
    uint32_t* const vm = static_cast<uint32_t*>(d->vmask);
    uint32_t* const bits = own ? vm : c.out;
    uint32_t* const list = pass2 ? vm + ns * words : nullptr;
    uint32_t* const pairbits = pass2 ? list + 1 + ns : nullptr;
    uint32_t* const out = rdev >= 0 ? c.out : c.locate ? vm + ns * words + pair_words : vm;
    if ((e = hipMemsetAsync(bits, 0, work_bytes + (pass2 ? sizeof(uint32_t) : 0), st)) != hipSuccess)
        return hip_fail(e, "hipMemsetAsync (result words)");
    thread_local std::vector<uint8_t> P, Q;
    P.resize(size_t(cc) * k);
    Q.resize(size_t(cc) * k);
    int rc = verify_rows(code, c.nums, c.nb, P.data());
    const bool hyp = c.locate && cc >= 2;
    if (!rc && hyp) locate_rows(P.data(), k, cc, Q.data());
    // with one check no verdict is a slot: nothing to heal, and the location is all there is
    const bool heal = c.heal && hyp;
    RaggedScrubStaged staged;
    const uint64_t* const sizes = reinterpret_cast<const uint64_t*>(c.sizes);
    const uint64_t* const soff = reinterpret_cast<const uint64_t*>(c.soff);
    const auto unfit = [&](unsigned checks, uint32_t* to) {
        ++t_launches;
        const hipError_t ue = launch_ragged_unfit(sizes, soff, ns, static_cast<uint32_t>(c.nb), c.sbs, c.src_bytes,
                                                  checks, to, st);
        return ue == hipSuccess ? int(FEC_OK) : hip_fail(ue, "launch_ragged_unfit");
    };
    // a verify's marks follow the clearing and precede the block kernel, which only ORs
    if (!rc && !c.locate && ddev >= 0) rc = unfit(cc, bits);
    if (!rc) {
        RaggedScrubSpec g;
        g.k = k;
        g.c = cc;
        g.P = P.data();
        g.Q = hyp ? Q.data() : nullptr;
        g.src = mem.z[0];
        g.bytes = c.src_bytes;
        g.bstride = c.sbs;
        g.sizes = sizes;
        g.off = soff;
        g.desc_host = ddev < 0;
        g.nstripes = ns;
        g.bits = bits;
        g.words = words;
        g.xbit = xbit;
        g.keep = heal || pass2 ? &staged : nullptr;
        ++t_launches;
        if ((e = launch_ragged_scrub(g, st)) != hipSuccess) rc = hip_fail(e, "launch_ragged_scrub");
    }
    if (!rc && c.locate) {
        // the block-reading kernel stays fec_last_kernel_name()'s answer
        ++t_launches;
        if (c.pairs) {
            // both planes, and (pass2) every MANY stripe onto the dirty list
            if ((e = launch_locate2_finish(bits, words, k, cc, ns, out, list, pairbits, st)) != hipSuccess)
                rc = hip_fail(e, "launch_locate2_finish");
        } else if ((e = launch_locate_finish(bits, words, k, cc, ns, out, st)) != hipSuccess) {
            rc = hip_fail(e, "launch_locate_finish");
        }
        // Overwrites the verdict (plane 0) of what was not read.  Such a stripe has no bit set, so
        // locate2_finish called it CLEAN and it cannot be on the dirty list: the pair pass never sees it.
        if (!rc && ddev >= 0) rc = unfit(0, out);
    }
    if (!rc && heal && staged.slot) {
        // row h of the nb x k correction matrix rebuilds slot h, over the verdict words in device
        // memory and the descriptors the location staged (mem.z[0] is the caller's writable blocks)
        thread_local std::vector<uint8_t> R;
        R.resize(c.nb * k);
        correct_rows(P.data(), k, cc, R.data());
        RaggedCorrectSpec cs;
        cs.k = k;
        cs.nb = static_cast<uint32_t>(c.nb);
        cs.rows = R.data();
        cs.blocks = const_cast<uint8_t*>(mem.z[0]);
        cs.bytes = c.src_bytes;
        cs.bstride = c.sbs;
        cs.nstripes = ns;
        cs.verdict = out;
        cs.staged = staged;
        ++t_launches;
        if ((e = launch_ragged_correct(cs, st)) != hipSuccess) rc = hip_fail(e, "launch_ragged_correct");
    }
    if (!rc && pass2 && staged.slot) {
        // plane 0 still reads MANY for the listed stripes: the pair pass names (a, b) and, with heal,
        // rewrites them, over the descriptors the location staged.  (No slot: nothing was read, the
        // list is empty.)  The host reads neither the list nor a verdict.
        PairRecs recs;
        rc = recs.build(P.data(), k, cc, c.heal, c.fn);
        PairsRaggedSpec ps;
        ps.k = k;
        ps.c = cc;
        ps.P = P.data();
        ps.pivots = recs.pivots;
        ps.sources = recs.sources;
        ps.crows = recs.crows;
        ps.blocks = const_cast<uint8_t*>(mem.z[0]);
        ps.bytes = c.src_bytes;
        ps.bstride = c.sbs;
        ps.sizes = staged.sizes;
        ps.off = staged.off;
        ps.nstripes = ns;
        ps.list = list;
        ps.pairbits = pairbits;
        ps.culprit = out;
        if (!rc) {
            t_launches += c.heal ? 3 : 2;
            if ((e = launch_pairs_ragged(ps, st)) != hipSuccess) rc = hip_fail(e, "launch_pairs_ragged");
        }
    }
    ragged_scrub_release(staged, st);
    if (!rc && rdev < 0 && (e = hipMemcpyAsync(c.out, out, out_bytes, hipMemcpyDeviceToHost, st)) != hipSuccess)
        rc = hip_fail(e, "hipMemcpyAsync D2H (result words)");
    order.release();
    if (rc) return rc;
    if ((rdev < 0 || !(c.flags & FEC_FLAG_ASYNC)) && (e = hipStreamSynchronize(st)) != hipSuccess)
        return hip_fail(e, "hipStreamSynchronize");
    return set_status(FEC_OK);
}

// Every other shape: runs of consecutive stripes of one size whose offset
// advances by a constant, each run one uniform verify / locate over the result
// words at + s0 * W or + s0 (run_ragged's cut for wide codes).  Device-side
// arrays are first copied to the host, which synchronises the stream.
int run_ragged_scrub_runs(const fec_t* code, const ScrubCall& c, int ddev, int rdev, BatchMem& mem) {
    const unsigned k = code->k, cc = static_cast<unsigned>(c.nb - k), cw = (cc + 31) / 32;
    const size_t ns = c.nstripes, W = c.locate ? 1 : cw;
    hipStream_t st = mem.st;
    hipError_t e;
    RaggedArgs d = ragged_args(c);
    if (fetch_desc(d, ddev, -1, st)) return t_status;
    // not live: empty, or (device-side arrays) it does not fit: not read
    const auto live = [&](size_t s) { return d.sizes[s] && ragged_stripe_fits(d, s); };
    // every word cleared (a location: CLEAN), then the marks of what will not be read
    const size_t out_bytes = ns * W * sizeof(uint32_t);
    const int fill = c.locate ? 0xFF : 0;
    if (rdev >= 0) {
        if ((e = hipMemsetAsync(c.out, fill, out_bytes, st)) != hipSuccess)
            return hip_fail(e, "hipMemsetAsync (result words)");
        if (ddev >= 0) {
            ++t_launches;
            e = launch_ragged_unfit(reinterpret_cast<const uint64_t*>(c.sizes),
                                    reinterpret_cast<const uint64_t*>(c.soff), ns, static_cast<uint32_t>(c.nb), c.sbs,
                                    c.src_bytes, c.locate ? 0 : cc, c.out, st);
            if (e != hipSuccess) return hip_fail(e, "launch_ragged_unfit");
        }
        // plane 1 of a pair call: NONE everywhere; a run's locate2_finish writes its own stripes again
        if (c.pairs && (e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c.out + ns),
                                              static_cast<int>(FEC_LOCATE_NONE), ns, st)) != hipSuccess)
            return hip_fail(e, "hipMemsetD32Async (plane 1)");
    } else {
        std::memset(c.out, fill, out_bytes);
        if (c.pairs) std::fill(c.out + ns, c.out + 2 * ns, unsigned(FEC_LOCATE_NONE));
        for (size_t s = 0; s < ns; ++s) {
            if (!d.sizes[s] || live(s)) continue;
            if (c.locate)
                c.out[s] = FEC_LOCATE_UNFIT;
            else
                for (unsigned i = 0; i < cw; ++i)
                    c.out[s * cw + i] = cc - 32 * i >= 32 ? ~0u : (1u << (cc - 32 * i)) - 1u;
        }
    }
    const unsigned jf = (c.flags & FEC_FLAG_LIBRARY_STREAM) | FEC_FLAG_ASYNC;
    if (for_each_ragged_run(
            d, live, [](size_t, size_t) { return true; }, [&](size_t s0, size_t s1, const size_t* step) {
                const size_t sz = d.sizes[s0], bs = c.sbs ? c.sbs : sz;
                const gf* const src = c.src + d.off[0][s0];
                return c.locate ? run_locate(code, src, bs, step[0], c.nums, c.nb, sz, s1 - s0, c.out + s0, c.stream,
                                             jf, c.fn, c.heal, c.pairs, c.pairs ? ns : 0)
                                : run_verify(code, src, bs, step[0], c.nums, c.nb, sz, s1 - s0, c.out + s0 * cw,
                                             c.stream, jf);
            }))
        return t_status;
    if (!(c.flags & FEC_FLAG_ASYNC) && (e = hipStreamSynchronize(st)) != hipSuccess)
        return hip_fail(e, "hipStreamSynchronize");
    return set_status(FEC_OK);
}

int ragged_scrub(const fec_t* code, const ScrubCall& c) {
    int ddev = -1;
    if (check_ragged_scrub(code, c, &ddev)) return t_status;
    if (c.nstripes == 0) return set_status(FEC_OK);
    if (!gpu_available()) return no_gpu();
    const unsigned k = code->k, cc = static_cast<unsigned>(c.nb - k);
    const char* const out_name = c.locate ? "culprit" : "mismatch";
    const int rdev = pointer_device(c.out);
    // device memory on one device, or page-locked host memory (read in place)
    const BatchBuf buf = {c.src, c.src_bytes, c.arena()};
    BatchMem mem;
    if (resolve_batch(mem, c.fn, &buf, 1, out_name, rdev, c.stream, c.flags, kCaptureRagged)) return t_status;
    if (ddev >= 0 && ddev != mem.dev)
        return set_status(FEC_EINVAL, "%s: sizes lives on device %d, the blocks on device %d", c.fn, ddev, mem.dev);
    if (k <= kMixedMaxK && (!c.locate || cc <= 8)) return run_ragged_scrub_fused(code, c, ddev, rdev, mem);
    return run_ragged_scrub_runs(code, c, ddev, rdev, mem);
}
}  // namespace

FEC_API int fec_verify_batch_ragged(const fec_t* code, const gf* src, size_t src_bytes, size_t src_block_stride,
                                    const unsigned long long* src_offsets, const unsigned long long* sizes,
                                    const unsigned* block_nums, size_t num_block_nums, size_t nstripes,
                                    unsigned* mismatch, void* stream, unsigned flags) {
    const ScrubCall c{"fec_verify_batch_ragged", false, src, src_bytes, src_block_stride, src_offsets, sizes,
                      block_nums, num_block_nums, nstripes, mismatch, stream, flags};
    return guarded([&] { return ragged_scrub(code, c); });
}

FEC_API int fec_locate_batch_ragged(const fec_t* code, const gf* src, size_t src_bytes, size_t src_block_stride,
                                    const unsigned long long* src_offsets, const unsigned long long* sizes,
                                    const unsigned* block_nums, size_t num_block_nums, size_t nstripes,
                                    unsigned* culprit, void* stream, unsigned flags) {
    const ScrubCall c{"fec_locate_batch_ragged", true, src, src_bytes, src_block_stride, src_offsets, sizes,
                      block_nums, num_block_nums, nstripes, culprit, stream, flags};
    return guarded([&] { return ragged_scrub(code, c); });
}

FEC_API int fec_correct_batch_ragged(const fec_t* code, gf* blocks, size_t bytes, size_t block_stride,
                                     const unsigned long long* offsets, const unsigned long long* sizes,
                                     const unsigned* block_nums, size_t num_block_nums, size_t nstripes,
                                     unsigned* culprit, void* stream, unsigned flags) {
    const ScrubCall c{"fec_correct_batch_ragged", true, blocks, bytes, block_stride, offsets, sizes,
                      block_nums, num_block_nums, nstripes, culprit, stream, flags, true};
    return guarded([&] { return ragged_scrub(code, c); });
}

// ---- batched in-place correction: scrub, locate and heal in one call ------------------------
FEC_API int fec_correct_rows(const fec_t* code, const unsigned* block_nums, size_t num_block_nums, gf* rows) {
    return rows_from_P(code, block_nums, num_block_nums, rows, correct_rows);
}

FEC_API int fec_correct_batch(const fec_t* code, gf* blocks, size_t block_stride, size_t stripe_stride,
                              const unsigned* block_nums, size_t num_block_nums, size_t sz, size_t nstripes,
                              unsigned* culprit, void* stream, unsigned flags) {
    // every check that needs no GPU comes first
    if (check_verify_call(code, blocks, "blocks", block_nums, num_block_nums, culprit, "culprit")) return t_status;
    if (nstripes == 0) return set_status(FEC_OK);
    return guarded([&] {
        return run_locate(code, blocks, block_stride, stripe_stride, block_nums, num_block_nums, sz, nstripes, culprit,
                          stream, flags, "fec_correct_batch", true);
    });
}

// ---- two corrupt blocks per stripe ---------------------------------------------------------
namespace {
// The checks of fec_locate2_rows / fec_correct2_rows after the block numbers': the pair, then the checks it needs.
int check_pair(size_t nb, unsigned k, unsigned a, unsigned b, unsigned cmin, const char* fn) {
    if (a >= b || b >= nb)
        return set_status(FEC_EINVAL, "%s: (a, b) = (%u, %u) is no pair of slots a < b < %zu", fn, a, b, nb);
    if (nb - k < cmin)
        return set_status(FEC_EINVAL, "%s: %zu checks per stripe, a pair needs at least %u", fn, nb - k, cmin);
    return FEC_OK;
}
}  // namespace

FEC_API int fec_locate2_rows(const fec_t* code, const unsigned* block_nums, size_t num_block_nums, unsigned a,
                             unsigned b, gf* rows) {
    if (check_verify_call(code, nullptr, nullptr, block_nums, num_block_nums, rows, "rows")) return t_status;
    if (check_pair(num_block_nums, code->k, a, b, 4, "fec_locate2_rows")) return t_status;
    return guarded([&] {
        const unsigned k = code->k, c = static_cast<unsigned>(num_block_nums - k);
        thread_local std::vector<uint8_t> P, piv;
        P.resize(size_t(c) * k);
        piv.resize(2 + 3 * size_t(c - 2));
        if (verify_rows(code, block_nums, num_block_nums, P.data())) return t_status;
        if (!pair_pivots(P.data(), k, c, a, b, piv.data()))
            return set_status(FEC_ESINGULAR, "fec_locate2_rows: slots %u and %u have dependent check columns", a, b);
        std::memset(rows, 0, size_t(c - 2) * c);
        for (unsigned m = 0; m + 2 < c; ++m) {
            gf* const row = rows + size_t(m) * c;
            row[piv[2 + 3 * m]] = 1;
            row[piv[0]] = piv[2 + 3 * m + 1];
            row[piv[1]] = piv[2 + 3 * m + 2];
        }
        return set_status(FEC_OK);
    });
}

FEC_API int fec_correct2_rows(const fec_t* code, const unsigned* block_nums, size_t num_block_nums, unsigned a,
                              unsigned b, unsigned* sources, gf* rows) {
    if (check_verify_call(code, nullptr, nullptr, block_nums, num_block_nums, rows, "rows")) return t_status;
    if (!sources) return set_status(FEC_EINVAL, "sources is NULL");
    if (check_pair(num_block_nums, code->k, a, b, 2, "fec_correct2_rows")) return t_status;
    return guarded([&] {
        const unsigned k = code->k, c = static_cast<unsigned>(num_block_nums - k);
        thread_local std::vector<uint8_t> P;
        P.resize(size_t(c) * k);
        if (verify_rows(code, block_nums, num_block_nums, P.data())) return t_status;
        static_assert(sizeof(unsigned) == sizeof(uint32_t), "source slots are 32-bit words");
        pair_correct_rows(P.data(), k, a, b, reinterpret_cast<uint32_t*>(sources), rows);
        return set_status(FEC_OK);
    });
}

FEC_API int fec_locate2_batch(const fec_t* code, const gf* src, size_t src_block_stride, size_t src_stripe_stride,
                              const unsigned* block_nums, size_t num_block_nums, size_t sz, size_t nstripes,
                              unsigned* culprit, void* stream, unsigned flags) {
    // every check that needs no GPU comes first
    if (check_verify_call(code, src, "src", block_nums, num_block_nums, culprit, "culprit")) return t_status;
    if (nstripes == 0) return set_status(FEC_OK);
    return guarded([&] {
        return run_locate(code, src, src_block_stride, src_stripe_stride, block_nums, num_block_nums, sz, nstripes,
                          culprit, stream, flags, "fec_locate2_batch", false, true);
    });
}

FEC_API int fec_correct2_batch(const fec_t* code, gf* blocks, size_t block_stride, size_t stripe_stride,
                               const unsigned* block_nums, size_t num_block_nums, size_t sz, size_t nstripes,
                               unsigned* culprit, void* stream, unsigned flags) {
    // every check that needs no GPU comes first
    if (check_verify_call(code, blocks, "blocks", block_nums, num_block_nums, culprit, "culprit")) return t_status;
    if (nstripes == 0) return set_status(FEC_OK);
    return guarded([&] {
        return run_locate(code, blocks, block_stride, stripe_stride, block_nums, num_block_nums, sz, nstripes, culprit,
                          stream, flags, "fec_correct2_batch", true, true);
    });
}

// The ragged forms: the ragged location's checks, paths and staging, two planes and the pair pass behind it.
FEC_API int fec_locate2_batch_ragged(const fec_t* code, const gf* src, size_t src_bytes, size_t src_block_stride,
                                     const unsigned long long* src_offsets, const unsigned long long* sizes,
                                     const unsigned* block_nums, size_t num_block_nums, size_t nstripes,
                                     unsigned* culprit, void* stream, unsigned flags) {
    const ScrubCall c{"fec_locate2_batch_ragged", true, src, src_bytes, src_block_stride, src_offsets, sizes,
                      block_nums, num_block_nums, nstripes, culprit, stream, flags, false, true};
    return guarded([&] { return ragged_scrub(code, c); });
}

FEC_API int fec_correct2_batch_ragged(const fec_t* code, gf* blocks, size_t bytes, size_t block_stride,
                                      const unsigned long long* offsets, const unsigned long long* sizes,
                                      const unsigned* block_nums, size_t num_block_nums, size_t nstripes,
                                      unsigned* culprit, void* stream, unsigned flags) {
    const ScrubCall c{"fec_correct2_batch_ragged", true, blocks, bytes, block_stride, offsets, sizes,
                      block_nums, num_block_nums, nstripes, culprit, stream, flags, true, true};
    return guarded([&] { return ragged_scrub(code, c); });
}

// ---- batched repair: any lost blocks of every stripe -----------------------------------
namespace {
// The checks of np repair patterns, in the documented order: every present
// number's range, then duplicates among a pattern's present numbers, then the
// targets (a block number or FEC_REPAIR_NONE).
int check_repair_patterns(const fec_t* code, const unsigned* present, const unsigned* targets, size_t nt, size_t np) {
    const unsigned k = code->k;
    for (size_t p = 0; p < np; ++p)
        for (unsigned j = 0; j < k; ++j)
            if (present[p * k + j] >= code->n)
                return set_status(FEC_EINVAL, "pattern %zu: block number %u out of range (n = %u)", p,
                                  present[p * k + j], unsigned(code->n));
    for (size_t p = 0; p < np; ++p)
        if (check_pattern(code, present + p * k, p)) return t_status;
    for (size_t p = 0; p < np; ++p)
        for (size_t i = 0; i < nt; ++i) {
            const unsigned t = targets[p * nt + i];
            if (t != FEC_REPAIR_NONE && t >= code->n)
                return set_status(FEC_EINVAL, "pattern %zu: target %u is neither a block number (n = %u) nor "
                                              "FEC_REPAIR_NONE", p, t, unsigned(code->n));
        }
    return FEC_OK;
}

// One pattern's nt x k matrix: row i = E[targets[i]] . inverse(E[present]), a
// FEC_REPAIR_NONE row all zeros; *mask (may be null) gets bit i for every other row.
int repair_rows(const fec_t* code, const unsigned* present, const unsigned* targets, size_t nt, uint8_t* rows,
                uint32_t* mask) {
    const unsigned k = code->k;
    thread_local std::vector<uint8_t> inv;
    inv.resize(size_t(k) * k);
    if (mixed_rows(code, present, inv.data())) return t_status;
    uint32_t live = 0;
    for (size_t i = 0; i < nt; ++i) {
        if (targets[i] == FEC_REPAIR_NONE) {
            std::memset(rows + i * k, 0, k);
        } else {
            enc_row_times(code, targets[i], inv.data(), rows + i * k);
            live |= 1u << i;
        }
    }
    if (mask) *mask = live;
    return FEC_OK;
}

// The live rows of one pattern as ONE shared-matrix application over nstripes
// stripes (whatever kernel apply_matrix picks; a block-major batch collapses
// into one long stripe as in fec_encode_batch).  Rows whose mask bit is clear
// are dropped from the launch, so their outputs are not touched.
int repair_shared(const uint8_t* rows, uint32_t mask, unsigned k, size_t nt, const gf* src, size_t sbs, size_t sss,
                  gf* dst, size_t dbs, size_t dss, size_t sz, size_t nstripes, hipStream_t st) {
    thread_local std::vector<uint8_t> coef;
    coef.resize(nt * k);
    const uint8_t* in[kMaxWideIn];
    uint8_t* out[kRepairMaxRows];
    unsigned r = 0;
    for (size_t i = 0; i < nt; ++i)
        if ((mask >> i) & 1u) {
            std::memcpy(&coef[size_t(r) * k], rows + i * k, k);
            out[r++] = dst + i * dbs;
        }
    if (!r) return FEC_OK;
    for (unsigned j = 0; j < k; ++j) in[j] = src + j * sbs;
    batch_geometry(k, r, sbs, sss, dbs, dss, 0, sz, nstripes);
    return apply_matrix(coef.data(), k, r, in, out, sz, nstripes, sss, dss, st);
}

int run_repair(const fec_t* code, const gf* src, size_t sbs, size_t sss, gf* dst, size_t dbs, size_t dss,
               const unsigned* present, const unsigned* targets, size_t nt, size_t npatterns,
               const unsigned* pattern_of, int idev, size_t sz, size_t nstripes, void* stream, unsigned flags) {
    const unsigned k = code->k;
    if (nstripes >= (size_t(1) << 32)) return set_status(FEC_EINVAL, "%zu stripes: a call takes fewer than 2^32", nstripes);
    // device memory on one device, or page-locked host memory (read and written in place);
    // with ids the pattern tables are uploaded, so the call cannot be captured
    const BatchBuf bufs[2] = {{src, (nstripes - 1) * sss + (k - 1) * sbs + sz, "src"},
                              {dst, (nstripes - 1) * dss + (nt - 1) * dbs + sz, "dst"}};
    BatchMem mem;
    if (resolve_batch(mem, "fec_repair_batch", bufs, 2, "pattern_of", idev, stream, flags,
                      pattern_of ? kCaptureTables : nullptr))
        return t_status;
    const gf* const zsrc = mem.z[0];
    gf* const zdst = const_cast<gf*>(mem.z[1]);
    hipStream_t st = mem.st;
    hipError_t e;
    thread_local std::vector<uint8_t> rows;
    thread_local std::vector<uint32_t> masks;
    bool runs = false;
    if (!pattern_of) {
        // one pattern for every stripe: a shared-matrix application, no new kernel
        rows.resize(nt * k);
        uint32_t mask = 0;
        if (repair_rows(code, present, targets, nt, rows.data(), &mask)) return t_status;
        if (repair_shared(rows.data(), mask, k, nt, zsrc, sbs, sss, zdst, dbs, dss, sz, nstripes, st)) return t_status;
    } else if (k <= kMixedMaxK || fused_mixed_shape(k, nt, sz, npatterns, mem)) {
        rows.resize(npatterns * nt * k);
        masks.resize(npatterns);
        for (size_t p = 0; p < npatterns; ++p)
            if (repair_rows(code, present + p * k, targets + p * nt, nt, &rows[p * nt * k], &masks[p]))
                return t_status;
        const uint8_t* in[kMaxIn];
        uint8_t* out[kRepairMaxRows];
        for (unsigned j = 0; j < k; ++j) in[j] = zsrc + j * sbs;
        for (size_t i = 0; i < nt; ++i) out[i] = zdst + i * dbs;
        RepairSpec r;
        r.k = k;
        r.t = static_cast<uint32_t>(nt);
        r.rows = rows.data();
        r.masks = masks.data();
        r.npatterns = static_cast<uint32_t>(npatterns);
        r.ids_host = idev < 0 ? pattern_of : nullptr;
        r.ids_dev = idev < 0 ? nullptr : pattern_of;
        r.in = in;
        r.out = out;
        r.sz = sz;
        r.nstripes = nstripes;
        r.in_sstride = sss;
        r.out_sstride = dss;
        ++t_launches;
        e = launch_repair(r, st);
        if (e == hipErrorNotSupported && k > kMixedMaxK)
            runs = true;  // the launch declined with nothing enqueued: the run path
        else if (e != hipSuccess)
            return hip_fail(e, "launch_repair");
    } else {
        runs = true;
    }
    if (runs) {
        // what the one launch does not take: each run one shared-matrix application of its pattern's live rows
        typedef std::pair<std::vector<uint8_t>, uint32_t> RowsAndMask;
        if (for_each_id_run<RowsAndMask>(
                pattern_of, idev, nstripes, npatterns, st,
                [&](unsigned id, RowsAndMask& pr) {
                    pr.first.resize(nt * k);
                    return repair_rows(code, present + size_t(id) * k, targets + size_t(id) * nt, nt,
                                       pr.first.data(), &pr.second);
                },
                [&](const RowsAndMask& pr, size_t s0, size_t s1) {
                    return repair_shared(pr.first.data(), pr.second, k, nt, zsrc + s0 * sss, sbs, sss,
                                         zdst + s0 * dss, dbs, dss, sz, s1 - s0, st);
                }))
            return t_status;
    }
    if (!(flags & FEC_FLAG_ASYNC) && (e = hipStreamSynchronize(st)) != hipSuccess)
        return hip_fail(e, "hipStreamSynchronize");
    return set_status(FEC_OK);
}
}  // namespace

FEC_API int fec_repair_rows(const fec_t* code, const unsigned* present, const unsigned* targets, size_t ntargets,
                            gf* rows) {
    if (!valid_code(code)) return set_status(FEC_EINVAL, "invalid fec_t");
    if (!present) return set_status(FEC_EINVAL, "present is NULL");
    if (!targets) return set_status(FEC_EINVAL, "targets is NULL");
    if (!rows) return set_status(FEC_EINVAL, "rows is NULL");
    if (ntargets == 0 || ntargets > kRepairMaxRows)
        return set_status(FEC_EINVAL, "ntargets is %zu: a pattern has between 1 and %u targets", ntargets,
                          unsigned(kRepairMaxRows));
    if (check_repair_patterns(code, present, targets, ntargets, 1)) return t_status;
    return guarded([&] {
        if (repair_rows(code, present, targets, ntargets, rows, nullptr)) return t_status;
        return set_status(FEC_OK);
    });
}

FEC_API int fec_repair_batch(const fec_t* code, const gf* src, size_t src_block_stride, size_t src_stripe_stride,
                             gf* dst, size_t dst_block_stride, size_t dst_stripe_stride, const unsigned* present,
                             const unsigned* targets, size_t ntargets, size_t npatterns, const unsigned* pattern_of,
                             size_t sz, size_t nstripes, void* stream, unsigned flags) {
    // every check that needs no GPU comes first
    if (!valid_code(code)) return set_status(FEC_EINVAL, "invalid fec_t");
    if (!src || !dst) return set_status(FEC_EINVAL, "NULL buffer");
    if (!present) return set_status(FEC_EINVAL, "present is NULL");
    if (!targets) return set_status(FEC_EINVAL, "targets is NULL");
    if (ntargets == 0 || ntargets > kRepairMaxRows)
        return set_status(FEC_EINVAL, "ntargets is %zu: a call takes between 1 and %u targets per stripe", ntargets,
                          unsigned(kRepairMaxRows));
    int idev = -1;
    if (check_patterns_and_ids(npatterns, nstripes, pattern_of, &idev, [&] {
            if (!pattern_of && npatterns != 1)
                return set_status(FEC_EINVAL, "pattern_of is NULL with %zu patterns: without ids every stripe uses "
                                              "pattern 0, so npatterns must be 1", npatterns);
            return check_repair_patterns(code, present, targets, ntargets, npatterns);
        }))
        return t_status;
    if (sz == 0 || nstripes == 0) return set_status(FEC_OK);
    return guarded([&] {
        return run_repair(code, src, src_block_stride, src_stripe_stride, dst, dst_block_stride, dst_stripe_stride,
                          present, targets, ntargets, npatterns, pattern_of, idev, sz, nstripes, stream, flags);
    });
}

// ---- batched parity update: changed primaries into the stored rows -----------------------
namespace {
// The checks fec_update_batch and fec_update_rows share, in the documented
// order: the code, the pointers (`what` names the first null one, or is null),
// then the stored rows' numbers -- their count, each one's range, duplicates.
int check_update_rows(const fec_t* code, const char* null_what, const unsigned* block_nums, size_t num) {
    if (!valid_code(code)) return set_status(FEC_EINVAL, "invalid fec_t");
    if (null_what) return set_status(FEC_EINVAL, "%s is NULL", null_what);
    if (num == 0 || num > code->n)
        return set_status(FEC_EINVAL, "num_block_nums is %zu: a call updates between 1 and n = %u stored rows", num,
                          unsigned(code->n));
    for (size_t i = 0; i < num; ++i)
        if (block_nums[i] >= code->n)
            return set_status(FEC_EINVAL, "block number %u out of range (n = %u)", block_nums[i], unsigned(code->n));
    unsigned char seen[256] = {};
    for (size_t i = 0; i < num; ++i) {
        if (seen[block_nums[i]]) return set_status(FEC_EINVAL, "duplicate block number %u", block_nums[i]);
        seen[block_nums[i]] = 1;
    }
    return FEC_OK;
}

int run_update(const fec_t* code, const gf* oldb, const gf* newb, size_t ibs, size_t iss, gf* rows, size_t rbs,
               size_t rss, const unsigned* block_nums, size_t nrows, const unsigned* changed, int cdev, size_t nc,
               size_t sz, size_t nstripes, void* stream, unsigned flags) {
    const unsigned k = code->k;
    // device memory on one device, or page-locked host memory (the rows updated in place);
    // the records are uploaded per call, so the call cannot be captured
    const size_t in_extent = (nstripes - 1) * iss + (nc - 1) * ibs + sz;
    const BatchBuf bufs[3] = {{newb, in_extent, "newb"},
                              {rows, (nstripes - 1) * rss + (nrows - 1) * rbs + sz, "rows"},
                              {oldb, in_extent, "oldb"}};
    BatchMem mem;
    if (resolve_batch(mem, "fec_update_batch", bufs, oldb ? 3 : 2, "changed", cdev, stream, flags, kCaptureTables))
        return t_status;
    hipStream_t st = mem.st;
    thread_local std::vector<uint8_t> coefs;
    coefs.resize(size_t(k) * nrows);
    for (unsigned j = 0; j < k; ++j)
        for (size_t i = 0; i < nrows; ++i) coefs[j * nrows + i] = code->enc_matrix[size_t(block_nums[i]) * k + j];
    uint8_t* out[kUpdateMaxRows];
    for (size_t i = 0; i < nrows; ++i) out[i] = const_cast<gf*>(mem.z[1]) + i * rbs;
    UpdateSpec u;
    u.k = k;
    u.nrows = static_cast<uint32_t>(nrows);
    u.c = static_cast<uint32_t>(nc);
    u.coefs = coefs.data();
    u.changed_host = cdev < 0 ? changed : nullptr;
    u.changed_dev = cdev < 0 ? nullptr : changed;
    u.oldb = oldb ? mem.z[2] : nullptr;
    u.newb = mem.z[0];
    u.in_bstride = ibs;
    u.in_sstride = iss;
    u.rows = out;
    u.row_sstride = rss;
    u.sz = sz;
    u.nstripes = nstripes;
    ++t_launches;
    hipError_t e = launch_update(u, st);
    if (e != hipSuccess) return hip_fail(e, "launch_update");
    if (!(flags & FEC_FLAG_ASYNC) && (e = hipStreamSynchronize(st)) != hipSuccess)
        return hip_fail(e, "hipStreamSynchronize");
    return set_status(FEC_OK);
}
}  // namespace

FEC_API int fec_update_rows(const fec_t* code, const unsigned* block_nums, size_t num_block_nums,
                            unsigned changed_block, gf* coefs) {
    if (check_update_rows(code, !block_nums ? "block_nums" : !coefs ? "coefs" : nullptr, block_nums, num_block_nums))
        return t_status;
    if (changed_block >= code->k)
        return set_status(FEC_EINVAL, "changed block %u is not a primary (k = %u)", changed_block, unsigned(code->k));
    for (size_t i = 0; i < num_block_nums; ++i)
        coefs[i] = code->enc_matrix[size_t(block_nums[i]) * code->k + changed_block];
    return set_status(FEC_OK);
}

FEC_API int fec_update_batch(const fec_t* code, const gf* oldb, const gf* newb, size_t in_block_stride,
                             size_t in_stripe_stride, gf* rows, size_t row_block_stride, size_t row_stripe_stride,
                             const unsigned* block_nums, size_t num_block_nums, const unsigned* changed,
                             size_t nchanged, size_t sz, size_t nstripes, void* stream, unsigned flags) {
    // every check that needs no GPU comes first
    static_assert(kUpdateMaxRows >= 256, "a call may name every block of the widest code");
    if (check_update_rows(code,
                          !newb ? "newb" : !rows ? "rows" : !block_nums ? "block_nums" : !changed ? "changed" : nullptr,
                          block_nums, num_block_nums))
        return t_status;
    if (nchanged == 0 || nchanged > kUpdateMaxSlots)
        return set_status(FEC_EINVAL, "nchanged is %zu: a stripe carries between 1 and %u changed blocks", nchanged,
                          unsigned(kUpdateMaxSlots));
    if (nstripes >= (size_t(1) << 32)) return set_status(FEC_EINVAL, "%zu stripes: a call takes fewer than 2^32", nstripes);
    const int ngpu = gpu_available();
    const int cdev = ngpu ? pointer_device(changed) : -1;
    if (cdev < 0)  // numbers in device memory cannot be checked: the kernel takes a bad one for FEC_UPDATE_NONE
        for (size_t s = 0; s < nstripes; ++s)
            for (size_t c = 0; c < nchanged; ++c) {
                const unsigned j = changed[s * nchanged + c];
                if (j != FEC_UPDATE_NONE && j >= code->k)
                    return set_status(FEC_EINVAL, "stripe %zu, slot %zu: changed block %u is neither a primary "
                                                  "(k = %u) nor FEC_UPDATE_NONE", s, c, j, unsigned(code->k));
            }
    if (!ngpu) return no_gpu();
    if (sz == 0 || nstripes == 0) return set_status(FEC_OK);
    return guarded([&] {
        return run_update(code, oldb, newb, in_block_stride, in_stripe_stride, rows, row_block_stride,
                          row_stripe_stride, block_nums, num_block_nums, changed, cdev, nchanged, sz, nstripes, stream,
                          flags);
    });
}

// ---- ragged repair: a size and a pattern per stripe ------------------------------------------
namespace {
int run_repair_ragged(const RaggedCall& c, const fec_t* code, const unsigned* present, const unsigned* targets,
                      size_t nt, size_t npatterns, const unsigned* pattern_of, int idev, int ddev) {
    const unsigned k = code->k;
    const size_t ns = c.nstripes;
    // device memory on one device, or page-locked host memory (read and written in place)
    const BatchBuf bufs[2] = {{c.src, c.src_bytes, "src"}, {c.dst, c.dst_bytes, "dst"}};
    BatchMem mem;
    if (resolve_batch(mem, c.fn, bufs, 2, "sizes", ddev, c.stream, c.flags, kCaptureRagged)) return t_status;
    if (idev >= 0 && idev != mem.dev)
        return set_status(FEC_EINVAL, "%s: pattern_of lives on device %d, the blocks on device %d", c.fn, idev,
                          mem.dev);
    const gf* const zsrc = mem.z[0];
    gf* const zdst = const_cast<gf*>(mem.z[1]);
    hipStream_t st = mem.st;
    hipError_t e;
    const unsigned r = static_cast<unsigned>(nt);
    if (k <= kMixedMaxK) {
        thread_local std::vector<uint8_t> rows;
        thread_local std::vector<uint32_t> masks;
        rows.resize(npatterns * nt * k);
        masks.resize(npatterns);
        for (size_t p = 0; p < npatterns; ++p)
            if (repair_rows(code, present + p * k, targets + p * nt, nt, &rows[p * nt * k], &masks[p]))
                return t_status;
        RaggedRepairSpec g;
        g.k = k;
        g.t = r;
        g.rows = rows.data();
        g.masks = masks.data();
        g.npatterns = static_cast<uint32_t>(npatterns);
        g.ids_host = pattern_of && idev < 0 ? pattern_of : nullptr;
        g.ids_dev = pattern_of && idev >= 0 ? pattern_of : nullptr;
        g.in = zsrc;
        g.out = zdst;
        g.in_bytes = c.src_bytes;
        g.out_bytes = c.dst_bytes;
        g.in_bstride = c.sbs;
        g.out_bstride = c.dbs;
        g.sizes = reinterpret_cast<const uint64_t*>(c.sizes);
        g.in_off = reinterpret_cast<const uint64_t*>(c.soff);
        g.out_off = reinterpret_cast<const uint64_t*>(c.doff);
        g.desc_host = ddev < 0;
        g.nstripes = ns;
        ++t_launches;
        if ((e = launch_ragged_repair(g, st)) != hipSuccess) return hip_fail(e, "launch_ragged_repair");
    } else {
        // wider codes: runs of consecutive stripes of one size and one pattern id whose two
        // offsets each advance by a constant, each run one shared-matrix application of that
        // pattern's live rows.  Device-side arrays come to the host first (a stream sync).
        RaggedArgs d = ragged_args(c, k, r);
        d.ids = pattern_of;
        if (fetch_desc(d, ddev, idev, st)) return t_status;
        const auto id_of = [&](size_t s) { return d.ids ? d.ids[s] : 0u; };
        typedef std::pair<std::vector<uint8_t>, uint32_t> RowsAndMask;
        std::unordered_map<unsigned, RowsAndMask> cache;
        // not live: empty, or (device-side arrays) unfit or a bad id: neither read nor written
        if (for_each_ragged_run(
                d, [&](size_t s) { return d.sizes[s] && id_of(s) < npatterns && ragged_stripe_fits(d, s); },
                [&](size_t s0, size_t s) { return id_of(s) == id_of(s0); },
                [&](size_t s0, size_t s1, const size_t* step) {
                    const size_t sz = d.sizes[s0];
                    const unsigned id = id_of(s0);
                    const auto ins = cache.try_emplace(id);
                    RowsAndMask& pr = ins.first->second;
                    if (ins.second) {
                        pr.first.resize(nt * k);
                        if (repair_rows(code, present + size_t(id) * k, targets + size_t(id) * nt, nt, pr.first.data(),
                                        &pr.second))
                            return t_status;
                    }
                    return repair_shared(pr.first.data(), pr.second, k, nt, zsrc + d.off[0][s0], c.sbs ? c.sbs : sz,
                                         step[0], zdst + d.off[1][s0], c.dbs ? c.dbs : sz, step[1], sz, s1 - s0, st);
                }))
            return t_status;
    }
    if (!(c.flags & FEC_FLAG_ASYNC) && (e = hipStreamSynchronize(st)) != hipSuccess)
        return hip_fail(e, "hipStreamSynchronize");
    return set_status(FEC_OK);
}
}  // namespace

FEC_API int fec_repair_batch_ragged(const fec_t* code, const gf* src, size_t src_bytes, size_t src_block_stride,
                                    const unsigned long long* src_offsets, gf* dst, size_t dst_bytes,
                                    size_t dst_block_stride, const unsigned long long* dst_offsets,
                                    const unsigned long long* sizes, const unsigned* present,
                                    const unsigned* targets, size_t ntargets, size_t npatterns,
                                    const unsigned* pattern_of, size_t nstripes, void* stream, unsigned flags) {
    const RaggedCall c{"fec_repair_batch_ragged", src,         src_bytes, src_block_stride, src_offsets, dst,
                       dst_bytes,                 dst_block_stride, dst_offsets, sizes,     nstripes,    stream,
                       flags};
    // fec_repair_batch's checks of the code and the pattern arguments, in its order
    const auto pattern_args = [&]() -> int {
        if (!valid_code(code)) return set_status(FEC_EINVAL, "invalid fec_t");
        if (!src || !dst) return set_status(FEC_EINVAL, "NULL buffer");
        if (!present) return set_status(FEC_EINVAL, "present is NULL");
        if (!targets) return set_status(FEC_EINVAL, "targets is NULL");
        if (ntargets == 0 || ntargets > kRepairMaxRows)
            return set_status(FEC_EINVAL, "ntargets is %zu: a call takes between 1 and %u targets per stripe",
                              ntargets, unsigned(kRepairMaxRows));
        if (npatterns == 0 && nstripes > 0)
            return set_status(FEC_EINVAL, "npatterns is 0: stripe 0 of %zu has no pattern", nstripes);
        if (npatterns > kMixedMaxPatterns)
            return set_status(FEC_EINVAL, "%zu patterns: a call takes at most %u", npatterns,
                              unsigned(kMixedMaxPatterns));
        if (!pattern_of && npatterns != 1)
            return set_status(FEC_EINVAL, "pattern_of is NULL with %zu patterns: without ids every stripe uses "
                                          "pattern 0, so npatterns must be 1", npatterns);
        return check_repair_patterns(code, present, targets, ntargets, npatterns);
    };
    if (pattern_args()) {
        const std::string msg = t_msg;
        return set_status(t_status, "%s: %s", c.fn, msg.c_str());
    }
    for (const auto& a : {std::make_pair(static_cast<const void*>(sizes), "sizes"),
                          std::make_pair(static_cast<const void*>(src_offsets), "src_offsets"),
                          std::make_pair(static_cast<const void*>(dst_offsets), "dst_offsets")})
        if (!a.first) return set_status(FEC_EINVAL, "%s: %s is NULL", c.fn, a.second);
    if (nstripes == 0) return set_status(FEC_OK);
    return guarded([&] {
        int ddev = -1;
        const RaggedArgs d = ragged_args(c, code->k, static_cast<unsigned>(ntargets));
        if (check_ragged_kinds(d, &ddev)) return t_status;
        const int idev = gpu_available() && pattern_of ? pointer_device(pattern_of) : -1;
        if (pattern_of && idev < 0)
            for (size_t s = 0; s < nstripes; ++s)
                if (pattern_of[s] >= npatterns)
                    return set_status(FEC_EINVAL, "%s: stripe %zu: pattern id %u out of range (npatterns = %zu)",
                                      c.fn, s, pattern_of[s], npatterns);
        if (check_ragged_fit(d, ddev)) return t_status;
        if (!gpu_available()) return no_gpu();
        return run_repair_ragged(c, code, present, targets, ntargets, npatterns, pattern_of, idev, ddev);
    });
}

// ---- ragged update: a size per stripe, changed primaries into the stored rows ---------------
namespace {
struct RaggedUpdateCall {
    const char* fn;
    const gf *oldb, *newb;
    size_t in_bytes, ibs;
    const unsigned long long* ioff;
    gf* rows;
    size_t row_bytes, rbs;
    const unsigned long long* roff;
    const unsigned long long* sizes;
    size_t nstripes;
    void* stream;
    unsigned flags;
};

RaggedArgs ragged_update_args(const RaggedUpdateCall& c, size_t nc, size_t nrows) {
    return RaggedArgs{c.fn,
                      "%s: sizes, in_offsets and row_offsets are of mixed memory kinds: all three in host memory, or "
                      "all three in device memory on the blocks' device",
                      2, {{"the inputs", "in_offsets", "in_bytes", c.in_bytes, c.ibs, nc},
                                {"the rows", "row_offsets", "row_bytes", c.row_bytes, c.rbs, nrows}},
                      c.nstripes, c.sizes, {c.ioff, c.roff}};
}

int run_update_ragged(const RaggedUpdateCall& c, const fec_t* code, const unsigned* block_nums, size_t nrows,
                      const unsigned* changed, int cdev, size_t nc, int ddev) {
    const unsigned k = code->k;
    // device memory on one device, or page-locked host memory (the rows updated in place)
    const BatchBuf bufs[3] = {{c.newb, c.in_bytes, "newb"}, {c.rows, c.row_bytes, "rows"}, {c.oldb, c.in_bytes, "oldb"}};
    BatchMem mem;
    if (resolve_batch(mem, c.fn, bufs, c.oldb ? 3 : 2, "sizes", ddev, c.stream, c.flags, kCaptureRagged))
        return t_status;
    if (cdev >= 0 && cdev != mem.dev)
        return set_status(FEC_EINVAL, "%s: changed lives on device %d, the blocks on device %d", c.fn, cdev, mem.dev);
    hipStream_t st = mem.st;
    thread_local std::vector<uint8_t> coefs;
    coefs.resize(size_t(k) * nrows);
    for (unsigned j = 0; j < k; ++j)
        for (size_t i = 0; i < nrows; ++i) coefs[j * nrows + i] = code->enc_matrix[size_t(block_nums[i]) * k + j];
    RaggedUpdateSpec u;
    u.k = k;
    u.nrows = static_cast<uint32_t>(nrows);
    u.c = static_cast<uint32_t>(nc);
    u.coefs = coefs.data();
    u.changed_host = cdev < 0 ? changed : nullptr;
    u.changed_dev = cdev < 0 ? nullptr : changed;
    u.oldb = c.oldb ? mem.z[2] : nullptr;
    u.newb = mem.z[0];
    u.rows = const_cast<gf*>(mem.z[1]);
    u.in_bytes = c.in_bytes;
    u.row_bytes = c.row_bytes;
    u.in_bstride = c.ibs;
    u.row_bstride = c.rbs;
    u.sizes = reinterpret_cast<const uint64_t*>(c.sizes);
    u.in_off = reinterpret_cast<const uint64_t*>(c.ioff);
    u.row_off = reinterpret_cast<const uint64_t*>(c.roff);
    u.desc_host = ddev < 0;
    u.nstripes = c.nstripes;
    ++t_launches;
    hipError_t e = launch_ragged_update(u, st);
    if (e != hipSuccess) return hip_fail(e, "launch_ragged_update");
    if (!(c.flags & FEC_FLAG_ASYNC) && (e = hipStreamSynchronize(st)) != hipSuccess)
        return hip_fail(e, "hipStreamSynchronize");
    return set_status(FEC_OK);
}
}  // namespace

FEC_API int fec_update_batch_ragged(const fec_t* code, const gf* oldb, const gf* newb, size_t in_bytes,
                                    size_t in_block_stride, const unsigned long long* in_offsets, gf* rows,
                                    size_t row_bytes, size_t row_block_stride,
                                    const unsigned long long* row_offsets, const unsigned long long* sizes,
                                    const unsigned* block_nums, size_t num_block_nums, const unsigned* changed,
                                    size_t nchanged, size_t nstripes, void* stream, unsigned flags) {
    const RaggedUpdateCall c{"fec_update_batch_ragged", oldb,        newb,  in_bytes, in_block_stride, in_offsets, rows,
                             row_bytes,                 row_block_stride, row_offsets, sizes, nstripes,   stream,
                             flags};
    // fec_update_batch's checks of the code, the pointers, the rows' numbers and the slot count, in its order
    const auto update_args = [&]() -> int {
        if (check_update_rows(
                code, !newb ? "newb" : !rows ? "rows" : !block_nums ? "block_nums" : !changed ? "changed" : nullptr,
                block_nums, num_block_nums))
            return t_status;
        if (nchanged == 0 || nchanged > kUpdateMaxSlots)
            return set_status(FEC_EINVAL, "nchanged is %zu: a stripe carries between 1 and %u changed blocks",
                              nchanged, unsigned(kUpdateMaxSlots));
        return FEC_OK;
    };
    if (update_args()) {
        const std::string msg = t_msg;
        return set_status(t_status, "%s: %s", c.fn, msg.c_str());
    }
    for (const auto& a : {std::make_pair(static_cast<const void*>(sizes), "sizes"),
                          std::make_pair(static_cast<const void*>(in_offsets), "in_offsets"),
                          std::make_pair(static_cast<const void*>(row_offsets), "row_offsets")})
        if (!a.first) return set_status(FEC_EINVAL, "%s: %s is NULL", c.fn, a.second);
    if (nstripes == 0) return set_status(FEC_OK);
    return guarded([&] {
        int ddev = -1;
        const RaggedArgs d = ragged_update_args(c, nchanged, num_block_nums);
        if (check_ragged_kinds(d, &ddev)) return t_status;
        const int cdev = gpu_available() ? pointer_device(changed) : -1;
        if (cdev < 0)  // numbers in device memory cannot be checked: the kernel takes a bad one for FEC_UPDATE_NONE
            for (size_t s = 0; s < nstripes; ++s)
                for (size_t i = 0; i < nchanged; ++i) {
                    const unsigned j = changed[s * nchanged + i];
                    if (j != FEC_UPDATE_NONE && j >= code->k)
                        return set_status(FEC_EINVAL, "%s: stripe %zu, slot %zu: changed block %u is neither a "
                                                      "primary (k = %u) nor FEC_UPDATE_NONE", c.fn, s, i, j,
                                          unsigned(code->k));
                }
        if (check_ragged_fit(d, ddev)) return t_status;
        if (!gpu_available()) return no_gpu();
        return run_update_ragged(c, code, block_nums, num_block_nums, changed, cdev, nchanged, ddev);
    });
}

// ---- pattern plans: the per-pattern work of fec_repair_batch done once --------------------
// Immutable after fec_repair_plan_new: the host-side rows and masks (the run
// path) and, in device memory of its own, the records the kernels read.
struct fec_repair_plan {
    unsigned long magic = 0;
    unsigned k = 0;
    size_t nt = 0, npatterns = 0;
    int device = -1;
    std::vector<uint8_t> rows;    // npatterns x nt x k
    std::vector<uint32_t> masks;  // npatterns live-row masks
    void* records = nullptr;      // device memory; null: every call takes the run path
};

namespace {
constexpr unsigned long kPlanMagic = 0x7265706c616eul;  // "replan"

bool valid_plan(const fec_repair_plan_t* p) { return p && p->magic == kPlanMagic; }

int run_repair_planned(const fec_repair_plan_t* plan, const gf* src, size_t sbs, size_t sss, gf* dst, size_t dbs,
                       size_t dss, const unsigned* pattern_of, int idev, size_t sz, size_t nstripes, void* stream,
                       unsigned flags) {
    static const char fn[] = "fec_repair_batch_planned";
    const unsigned k = plan->k;
    const size_t nt = plan->nt, npatterns = plan->npatterns;
    if (nstripes >= (size_t(1) << 32)) return set_status(FEC_EINVAL, "%zu stripes: a call takes fewer than 2^32", nstripes);
    const BatchBuf bufs[2] = {{src, (nstripes - 1) * sss + (k - 1) * sbs + sz, "src"},
                              {dst, (nstripes - 1) * dss + (nt - 1) * dbs + sz, "dst"}};
    BatchMem mem;
    if (resolve_batch(mem, fn, bufs, 2, "pattern_of", idev, stream, flags, nullptr)) return t_status;
    if ((mem.bdev[0] >= 0 || mem.bdev[1] >= 0 || idev >= 0) && mem.dev != plan->device)
        return set_status(FEC_EINVAL, "%s: the plan lives on device %d, the %s on device %d", fn, plan->device,
                          mem.bdev[0] >= 0 || mem.bdev[1] >= 0 ? "blocks" : "ids", mem.dev);
    const gf* const zsrc = mem.z[0];
    gf* const zdst = const_cast<gf*>(mem.z[1]);
    hipStream_t st = mem.st;
    hipError_t e;
    // one launch over the plan's records: the register kernels (any memory the
    // device sees) or, on device blocks, the mix form of the bit-sliced kernels
    bool one = plan->records && mem.dev == plan->device &&
               (k <= kMixedMaxK || (config().mixed_fused && mem.bdev[0] >= 0 && mem.bdev[1] >= 0 &&
                                    bsr_mix_ok(k, static_cast<uint32_t>(nt), sz)));
    // only that launch with the ids where they are touches nothing the library owns and reuses
    const bool capturing = stream_capturing(st);
    if (capturing && !(one && idev >= 0))
        return set_status(FEC_EINVAL, "%s: the stream is being captured into a graph (%s)", fn,
                          one ? "host-side ids are staged when the call is made" : kCaptureMemory);
    if (one) {
        const uint8_t* in[kMaxIn];
        uint8_t* out[kRepairMaxRows];
        for (unsigned j = 0; j < k; ++j) in[j] = zsrc + j * sbs;
        for (size_t i = 0; i < nt; ++i) out[i] = zdst + i * dbs;
        RepairSpec r;
        r.k = k;
        r.t = static_cast<uint32_t>(nt);
        r.rows = nullptr;
        r.masks = plan->masks.data();
        r.npatterns = static_cast<uint32_t>(npatterns);
        r.ids_host = idev < 0 ? pattern_of : nullptr;
        r.ids_dev = idev < 0 ? nullptr : pattern_of;
        r.in = in;
        r.out = out;
        r.sz = sz;
        r.nstripes = nstripes;
        r.in_sstride = sss;
        r.out_sstride = dss;
        ++t_launches;
        e = launch_repair_records(r, plan->records, st);
        if (e == hipErrorNotSupported && k > kMixedMaxK && !capturing)
            one = false;  // the launch declined with nothing enqueued: the run path
        else if (e != hipSuccess)
            return hip_fail(e, "launch_repair_records");
    }
    if (!one) {
        // the run path of fec_repair_batch, from the plan's host rows
        struct Ref {
            const uint8_t* rows;
            uint32_t mask;
        };
        if (for_each_id_run<Ref>(
                pattern_of, idev, nstripes, npatterns, st,
                [&](unsigned id, Ref& r) {
                    r.rows = &plan->rows[size_t(id) * nt * k];
                    r.mask = plan->masks[id];
                    return int(FEC_OK);
                },
                [&](const Ref& r, size_t s0, size_t s1) {
                    return repair_shared(r.rows, r.mask, k, nt, zsrc + s0 * sss, sbs, sss, zdst + s0 * dss, dbs, dss,
                                         sz, s1 - s0, st);
                }))
            return t_status;
    }
    if (!(flags & FEC_FLAG_ASYNC) && (e = hipStreamSynchronize(st)) != hipSuccess)
        return hip_fail(e, "hipStreamSynchronize");
    return set_status(FEC_OK);
}
}  // namespace

FEC_API int fec_repair_plan_new(const fec_t* code, const unsigned* present, const unsigned* targets, size_t ntargets,
                                size_t npatterns, int device, fec_repair_plan_t** plan) {
    // every check that needs no GPU comes first, in fec_repair_batch's order
    if (plan) *plan = nullptr;
    if (!valid_code(code)) return set_status(FEC_EINVAL, "invalid fec_t");
    if (!present) return set_status(FEC_EINVAL, "present is NULL");
    if (!targets) return set_status(FEC_EINVAL, "targets is NULL");
    if (!plan) return set_status(FEC_EINVAL, "plan is NULL");
    if (ntargets == 0 || ntargets > kRepairMaxRows)
        return set_status(FEC_EINVAL, "ntargets is %zu: a plan takes between 1 and %u targets per pattern", ntargets,
                          unsigned(kRepairMaxRows));
    if (npatterns == 0) return set_status(FEC_EINVAL, "npatterns is 0: a plan holds at least one pattern");
    if (npatterns > kMixedMaxPatterns)
        return set_status(FEC_EINVAL, "%zu patterns: a plan takes at most %u", npatterns, unsigned(kMixedMaxPatterns));
    if (check_repair_patterns(code, present, targets, ntargets, npatterns)) return t_status;
    const int ngpu = gpu_available();
    if (!ngpu) return set_status(FEC_ENODEV, "no GPU visible to HIP (the engine has no CPU path)");
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return set_status(FEC_ENODEV, "no current HIP device");
    if (device >= ngpu) return set_status(FEC_EINVAL, "device %d: HIP sees %d", device, ngpu);
    return guarded([&] {
        const unsigned k = code->k;
        std::unique_ptr<fec_repair_plan> p(new fec_repair_plan);
        p->k = k;
        p->nt = ntargets;
        p->npatterns = npatterns;
        p->device = device;
        p->rows.resize(npatterns * ntargets * k);
        p->masks.resize(npatterns);
        for (size_t q = 0; q < npatterns; ++q)
            if (repair_rows(code, present + q * k, targets + q * ntargets, ntargets, &p->rows[q * ntargets * k],
                            &p->masks[q]))
                return t_status;
        // the records, where a kernel reads them (k <= 32) and they stay within the cap
        const size_t bytes = repair_records_bytes(k, static_cast<uint32_t>(ntargets), npatterns);
        if (bytes && (k <= kMixedMaxK || bytes <= kBsrMixMaxBytes)) {
            DeviceGuard guard(device);
            std::vector<uint8_t> host(bytes);
            hipError_t e = repair_records_fill(host.data(), p->rows.data(), p->masks.data(), npatterns, k,
                                               static_cast<uint32_t>(ntargets));
            if (e == hipSuccess) {
                if ((e = hipMalloc(&p->records, bytes)) != hipSuccess)
                    return set_status(FEC_ENOMEM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
                if ((e = hipMemcpy(p->records, host.data(), bytes, hipMemcpyHostToDevice)) != hipSuccess) {
                    (void)hipFree(p->records);
                    return hip_fail(e, "hipMemcpy H2D (plan records)");
                }
            } else if (e != hipErrorNotSupported) {
                return hip_fail(e, "repair_records_fill");
            }  // no routine table on the device: no records, the run path
        }
        p->magic = kPlanMagic;
        *plan = p.release();
        return set_status(FEC_OK);
    });
}

FEC_API void fec_repair_plan_free(fec_repair_plan_t* plan) {
    if (!valid_plan(plan)) return;
    plan->magic = 0;
    if (plan->records) {
        DeviceGuard guard(plan->device);
        (void)hipFree(plan->records);
    }
    delete plan;
}

FEC_API int fec_repair_batch_planned(const fec_repair_plan_t* plan, const gf* src, size_t src_block_stride,
                                     size_t src_stripe_stride, gf* dst, size_t dst_block_stride,
                                     size_t dst_stripe_stride, const unsigned* pattern_of, size_t sz, size_t nstripes,
                                     void* stream, unsigned flags) {
    // every check that needs no GPU comes first
    if (!valid_plan(plan)) return set_status(FEC_EINVAL, "invalid fec_repair_plan_t");
    if (!src || !dst) return set_status(FEC_EINVAL, "NULL buffer");
    if (!pattern_of) return set_status(FEC_EINVAL, "pattern_of is NULL");
    int idev = -1;
    if (check_patterns_and_ids(plan->npatterns, nstripes, pattern_of, &idev, [] { return int(FEC_OK); }))
        return t_status;
    if (sz == 0 || nstripes == 0) return set_status(FEC_OK);
    return guarded([&] {
        return run_repair_planned(plan, src, src_block_stride, src_stripe_stride, dst, dst_block_stride,
                                  dst_stripe_stride, pattern_of, idev, sz, nstripes, stream, flags);
    });
}

namespace zfec_hip {
namespace {
// A fec_run_batch_jobs job resolved for a paired launch (register-kernel
// shapes: k <= 4, r <= 8).
struct PairJobSpec {
    uint8_t coef[4 * 8];
    unsigned k = 0, r = 0;
    const uint8_t* in[4];
    uint8_t* out[8];
    size_t sz = 0, nstripes = 0, sss = 0, dss = 0;
    int dev = -1;
};

// Resolve job j; *ok = false when it cannot share a launch (host memory,
// another shape, an empty job, more units than one launch takes).
int resolve_pair_job(const fec_batch_job& j, PairJobSpec& p, bool* ok) {
    *ok = false;
    const unsigned k = j.code->k;
    if (k > 4 || !j.sz || !j.nstripes || !j.src || !j.dst) return FEC_OK;
    if (j.kind == FEC_JOB_ENCODE) {
        if (j.num_nums == 0 || j.num_nums > 8) return FEC_OK;
        p.r = static_cast<unsigned>(j.num_nums);
        std::memcpy(p.coef, encode_rows(j.code, j.nums, j.num_nums), size_t(p.r) * k);
    } else {
        thread_local std::vector<uint8_t> rows;
        unsigned r = 0;
        if (decode_rows(j.code, j.nums, rows, r, (j.flags & FEC_FLAG_ALL_PRIMARIES) != 0)) return t_status;
        if (r == 0 || r > 8) return FEC_OK;
        p.r = r;
        std::memcpy(p.coef, rows.data(), size_t(r) * k);
    }
    p.k = k;
    const int sdev = pointer_device(j.src), ddev = pointer_device(j.dst);
    if (sdev < 0 || sdev != ddev) return FEC_OK;
    p.dev = sdev;
    p.sz = j.sz;
    p.nstripes = j.nstripes;
    p.sss = j.src_stripe_stride;
    p.dss = j.dst_stripe_stride;
    batch_geometry(k, p.r, j.src_block_stride, p.sss, j.dst_block_stride, p.dss, j.flags, p.sz, p.nstripes);
    // apply_matrix's one-launch condition
    const size_t cps = (p.sz + kMinChunk - 1) / kMinChunk, max_units = config().launch_units;
    if (cps > max_units || std::max<size_t>(1, max_units / cps) < p.nstripes) return FEC_OK;
    for (unsigned i = 0; i < k; ++i) p.in[i] = j.src + i * j.src_block_stride;
    for (unsigned i = 0; i < p.r; ++i) p.out[i] = j.dst + i * j.dst_block_stride;
    *ok = true;
    return FEC_OK;
}

ApplySpec pair_spec(const PairJobSpec& p) {
    ApplySpec a;
    a.coef = p.coef;
    a.coef_stride = p.k;
    a.k = p.k;
    a.r = p.r;
    a.in = p.in;
    a.out = p.out;
    a.sz = p.sz;
    a.nstripes = p.nstripes;
    a.in_sstride = p.sss;
    a.out_sstride = p.dss;
    a.accumulate = false;
    return a;
}

int job_failed(size_t i) {
    char msg[sizeof t_msg];
    snprintf(msg, sizeof msg, "%s", t_msg);
    return set_status(t_status, "job %zu: %s", i, msg);
}
}  // namespace
}  // namespace zfec_hip

FEC_API int fec_run_batch_jobs(const fec_batch_job* jobs, size_t njobs, void* stream, unsigned flags) {
    if (njobs && !jobs) return set_status(FEC_EINVAL, "jobs is NULL");
    for (size_t i = 0; i < njobs; ++i) {
        const fec_batch_job& j = jobs[i];
        if (!valid_code(j.code)) return set_status(FEC_EINVAL, "job %zu: invalid fec_t", i);
        if (j.kind != FEC_JOB_ENCODE && j.kind != FEC_JOB_DECODE)
            return set_status(FEC_EINVAL, "job %zu: kind %u is neither FEC_JOB_ENCODE nor FEC_JOB_DECODE", i, j.kind);
        if (j.kind == FEC_JOB_ENCODE && check_block_nums(j.code, j.nums, j.num_nums)) return job_failed(i);
    }
    if (!gpu_available()) return set_status(FEC_ENODEV, "no GPU visible to HIP (the engine has no CPU path)");
    return guarded([&] {
        const unsigned call = flags & (FEC_FLAG_ASYNC | FEC_FLAG_LIBRARY_STREAM);
        // every device a job ran on, each once (no cap: a synchronous call
        // must wait on all of them before it reports FEC_OK)
        std::vector<int> devs;
        auto note_dev = [&](int dev) {
            for (int d : devs)
                if (d == dev) return;
            devs.push_back(dev);
        };
        size_t i = 0;
        while (i < njobs) {
            if (i + 1 < njobs) {
                PairJobSpec a, b;
                bool oka = false, okb = false;
                if (resolve_pair_job(jobs[i], a, &oka)) return job_failed(i);
                if (oka && resolve_pair_job(jobs[i + 1], b, &okb)) return job_failed(i + 1);
                if (oka && okb && a.dev == b.dev && a.k == b.k) {
                    DeviceGuard guard(a.dev);
                    DevCtx* d = nullptr;
                    if (dev_ctx(a.dev, &d)) return t_status;
                    hipStream_t st = (flags & FEC_FLAG_LIBRARY_STREAM) ? d->stream : static_cast<hipStream_t>(stream);
                    const hipError_t e = launch_apply_pair(pair_spec(a), pair_spec(b), st);
                    if (e == hipSuccess) {
                        ++t_launches;
                        note_dev(a.dev);
                        i += 2;
                        continue;
                    }
                    if (e != hipErrorNotSupported) {
                        hip_fail(e, "launch_apply_pair");
                        return job_failed(i);
                    }
                }
            }
            const fec_batch_job& j = jobs[i];
            const unsigned jf = (j.flags & (FEC_FLAG_ROW_PADDING | FEC_FLAG_ALL_PRIMARIES)) | call | FEC_FLAG_ASYNC;
            const int st = j.kind == FEC_JOB_ENCODE
                               ? fec_encode_batch(j.code, j.src, j.src_block_stride, j.src_stripe_stride, j.dst,
                                                  j.dst_block_stride, j.dst_stripe_stride, j.nums, j.num_nums, j.sz,
                                                  j.nstripes, stream, jf)
                               : fec_decode_batch(j.code, j.src, j.src_block_stride, j.src_stripe_stride, j.dst,
                                                  j.dst_block_stride, j.dst_stripe_stride, j.nums, j.sz, j.nstripes,
                                                  stream, jf);
            if (st) return job_failed(i);
            int dev = pointer_device(j.src);
            if (dev < 0) dev = pointer_device(j.dst);
            if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = 0;
            note_dev(dev);
            ++i;
        }
        if (!(flags & FEC_FLAG_ASYNC)) {
            if (!(flags & FEC_FLAG_LIBRARY_STREAM) && stream) {
                const hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(stream));
                if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
            } else if (!(flags & FEC_FLAG_LIBRARY_STREAM)) {
                // the null stream: each job ran on its own device's null stream
                for (int dv : devs) {
                    DeviceGuard guard(dv);
                    const hipError_t e = hipStreamSynchronize(nullptr);
                    if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
                }
            } else {
                for (int dv : devs) {
                    DeviceGuard guard(dv);
                    DevCtx* d = nullptr;
                    if (dev_ctx(dv, &d)) return t_status;
                    const hipError_t e = hipStreamSynchronize(d->stream);
                    if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
                }
            }
        }
        return set_status(FEC_OK);
    });
}

// ============================================================================
// Several GPUs of one process: a batch's stripes are
// independent (zfec/fec.c:494-503 touches one column range of each block), so
// the batch is split into contiguous balanced stripe ranges, one per listed
// device, each run by a persistent host thread bound to that device with its
// own stream and staging slots -- the reference's only parallelism is the
// same thing on CPU threads (the GIL released around fec_encode,
// zfec/_fecmodule.c:221-223).  Host memory only: each GPU reads and writes
// its share over its own PCIe link; device-resident batches stay on their
// device (one fec_encode_batch per device).
// ============================================================================
namespace {

// One persistent thread per (device, position in the call's device list): the
// thread-local contexts (streams, pinned slots) it builds on first use are
// kept for later calls.
class DevWorker {
public:
    explicit DevWorker(int dev) : dev_(dev), th_([this] { loop(); }) {}
    void post(std::function<void()> fn) {
        {
            std::lock_guard<std::mutex> g(mu_);
            q_.push_back(std::move(fn));
        }
        cv_.notify_one();
    }

private:
    void loop() {
        (void)hipSetDevice(dev_);
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            cv_.wait(lk, [this] { return !q_.empty(); });
            std::function<void()> fn = std::move(q_.front());
            q_.pop_front();
            lk.unlock();
            fn();
            lk.lock();
        }
    }
    int dev_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<std::function<void()>> q_;
    std::thread th_;
};

DevWorker& dev_worker(int dev, size_t pos) {
    // lives for the process (workers may be parked at exit); a forked child
    // builds its own
    static std::mutex m;
    static std::map<std::pair<int, size_t>, DevWorker*>* workers = nullptr;
    static pid_t owner = 0;
    std::lock_guard<std::mutex> g(m);
    if (!workers || owner != getpid()) {
        workers = new std::map<std::pair<int, size_t>, DevWorker*>;
        owner = getpid();
    }
    DevWorker*& w = (*workers)[{dev, pos}];
    if (!w) w = new DevWorker(dev);
    return *w;
}

struct ShardResult {
    int status = FEC_OK;
    char msg[256] = "";
};

int run_batch_multi(const fec_t* code, const uint8_t* coef, unsigned r, const gf* src, size_t sbs, size_t sss,
                    gf* dst, size_t dbs, size_t dss, size_t sz, size_t nstripes, const int* devices, size_t ndev,
                    unsigned flags) {
    const int ngpu = gpu_available();
    if (!ngpu) return set_status(FEC_ENODEV, "no GPU visible to HIP (the engine has no CPU path)");
    if (!src || !dst) return set_status(FEC_EINVAL, "NULL buffer");
    if (!devices || ndev == 0) return set_status(FEC_EINVAL, "no devices listed");
    for (size_t d = 0; d < ndev; ++d)
        if (devices[d] < 0 || devices[d] >= ngpu)
            return set_status(FEC_EINVAL, "device %d out of range (%d visible)", devices[d], ngpu);
    if (pointer_device(src) >= 0 || pointer_device(dst) >= 0)
        return set_status(FEC_EINVAL,
                          "multi-device calls take host memory (device-resident batches: one call per device)");
    std::vector<ShardResult> res(ndev);
    std::mutex mu;
    std::condition_variable cv;
    // stripes [s0, s1) of shard d: balanced contiguous ranges (zfec_amd/shard.py shard_range)
    const size_t base = nstripes / ndev, extra = nstripes % ndev;
    const size_t shards = std::min(ndev, nstripes);  // the non-empty ones: d < nstripes
    size_t left = shards;  // shards not finished (or never posted); guarded by mu
    // The workers reference this frame (mu, cv, left, res): whatever happens
    // while posting (a thread that cannot be created, bad_alloc), the frame
    // stays until every posted shard has finished.
    int post_status = FEC_OK;
    char post_msg[sizeof t_msg] = "";
    for (size_t d = 0; d < shards; ++d) {
        const size_t s0 = d * base + std::min(d, extra), n = base + (d < extra ? 1 : 0);
        const gf* ps = src + s0 * sss;
        gf* pd = dst + s0 * dss;
        ShardResult* out = &res[d];
        const int dev = devices[d];
        const int pst = guarded([&] {
            dev_worker(dev, d).post([=, &mu, &cv, &left] {
                (void)hipSetDevice(dev);
                const int st = guarded([&] {
                    return run_batch(code, coef, r, ps, sbs, sss, pd, dbs, dss, sz, n, nullptr,
                                     (flags & ~FEC_FLAG_ASYNC) | FEC_FLAG_LIBRARY_STREAM);
                });
                out->status = st;
                if (st != FEC_OK) snprintf(out->msg, sizeof out->msg, "device %d: %s", dev, t_msg);
                std::lock_guard<std::mutex> g(mu);
                if (--left == 0) cv.notify_all();
            });
            return FEC_OK;
        });
        if (pst != FEC_OK) {  // shards d.. were never posted: take them off the count
            post_status = pst;
            snprintf(post_msg, sizeof post_msg, "%s", t_msg);
            std::lock_guard<std::mutex> g(mu);
            left -= shards - d;
            break;
        }
    }
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return left == 0; });
    }
    if (post_status != FEC_OK) return set_status(post_status, "%s", post_msg);
    for (const ShardResult& r0 : res)
        if (r0.status != FEC_OK) return set_status(r0.status, "%s", r0.msg);
    return set_status(FEC_OK);
}

}  // namespace

FEC_API int fec_encode_batch_multi(const fec_t* code, const gf* src, size_t src_block_stride,
                                   size_t src_stripe_stride, gf* dst, size_t dst_block_stride,
                                   size_t dst_stripe_stride, const unsigned* block_nums, size_t num_block_nums,
                                   size_t sz, size_t nstripes, const int* devices, size_t ndevices, unsigned flags) {
    if (!valid_code(code)) return set_status(FEC_EINVAL, "invalid fec_t");
    if (check_block_nums(code, block_nums, num_block_nums)) return t_status;
    if (num_block_nums == 0 || sz == 0 || nstripes == 0) return set_status(FEC_OK);
    return guarded([&] {
        return run_batch_multi(code, encode_rows(code, block_nums, num_block_nums),
                               static_cast<unsigned>(num_block_nums), src, src_block_stride, src_stripe_stride, dst,
                               dst_block_stride, dst_stripe_stride, sz, nstripes, devices, ndevices, flags);
    });
}

FEC_API int fec_decode_batch_multi(const fec_t* code, const gf* src, size_t src_block_stride,
                                   size_t src_stripe_stride, gf* dst, size_t dst_block_stride,
                                   size_t dst_stripe_stride, const unsigned* index, size_t sz, size_t nstripes,
                                   const int* devices, size_t ndevices, unsigned flags) {
    if (!valid_code(code)) return set_status(FEC_EINVAL, "invalid fec_t");
    thread_local std::vector<uint8_t> rows;
    unsigned r = 0;
    if (decode_rows(code, index, rows, r, (flags & FEC_FLAG_ALL_PRIMARIES) != 0)) return t_status;
    if (r == 0 || sz == 0 || nstripes == 0) return set_status(FEC_OK);
    return guarded([&] {
        return run_batch_multi(code, rows.data(), r, src, src_block_stride, src_stripe_stride, dst, dst_block_stride,
                               dst_stripe_stride, sz, nstripes, devices, ndevices, flags);
    });
}
