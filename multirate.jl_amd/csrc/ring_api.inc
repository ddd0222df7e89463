// ring_api.inc -- the host side of the resident ring consumer (mrhip_ring_*, include/multirate_hip.h); included by api.hip.
//
// The reference's streaming usage is a loop of filt(self, chunk) on one stateful FIRFilter (README.md:87-141).  As one launch per
// arriving chunk that loop is launch-bound on this chip for anything but large batches (13 us per 1e6-sample chunk of one channel
// round a kernel that needs 1.5 us of the machine).  A ring keeps ONE kernel resident: mrhip_ring_push plans the chunk on the host
// (closed form of the state recurrence, Filters.jl:558-571 -- so filt!'s return value is known at once) and writes a descriptor
// into pinned memory; the kernel's feeder wave fetches it, the chunk's grabs of steps are dealt to the resident workgroups next
// to those of the chunks before it, the history (shiftin!, support.jl:61-80) travels from chunk to chunk through slots in device
// memory, and the completion of every chunk is a flag the kernel raises in pinned memory (mrhip_ring_wait).  Filters the resident
// kernel is not instantiated for run the same interface as stream-ordered launches, one per chunk (resident == 0 in mrhip_ring_info).
#include <atomic>
#include <thread>

namespace mrhip {
bool opair_ring_available(const TypeKey &tk, bool fused, const PolyArgs &a);   // kernels_rational_opair.hip
}

struct mrhip_ring {
    mrhip_filter *f = nullptr;
    bool resident = false;
    hipStream_t stream = nullptr;
    // resident mode
    mrhip::RingHost *host = nullptr;          // pinned
    mrhip::RingHost *host_dev = nullptr;      // ... as the device sees it
    mrhip::RingDev *dev = nullptr;
    void *hist = nullptr;                     // kRingDepth history slots
    size_t slot_bytes = 0;
    mrhip::PolyArgs a{};
    mrhip::PairArgs pa{};
    dim3 block;
    size_t lds = 0;
    bool running = false;
    uint64_t epoch_base = 0;                  // chunks of earlier epochs (an epoch = one life of the resident kernel)
    uint64_t pushed = 0;                      // chunks pushed in this epoch
    uint64_t done_upto = 0;                   // every chunk below it is complete (this epoch)
    uint64_t tile_base = 0;
    int64_t phiIdx = 1, inputDeficit = 1;     // the stream state behind the last pushed chunk
    uint64_t idle_ticks = 0;
    int64_t stat_restarts = 0;
    int64_t stat_shrunk = 0;             // launches repeated with fewer workgroups (ring_launch)
    int xccs = 8;                        // XCDs of the device (hipDeviceAttributeNumberOfXccs)
    // per-chunk launches
    hipEvent_t ev[mrhip::kRingDepth] = {};
    uint64_t ev_seq[mrhip::kRingDepth] = {};
    uint64_t launched = 0;
};

namespace {

// ONE resident consumer per device: its workgroups are dealt tickets statically and must all be on the chip at once -- a second resident
// kernel beside it would leave workgroups of one of them waiting for a place while the others wait for their tickets' results.  A ring
// opened while another one is resident on the device runs as stream-ordered launches (same interface, same results).
std::mutex g_ring_mutex;
int g_resident_rings[64] = {};

int ring_launch(mrhip_ring *r)
{
    // Tickets are dealt statically (ticket t -> workgroup t mod G): EVERY workgroup of the grid must be on the chip.  The grid is what the
    // occupancy query says the chip holds -- with no slack: two workgroups on each of 256 CUs -- and that can be a few too many (the Float64
    // instantiation at 5//3, five channels: 509 of 512 started, the other three when the first left: profiles/r05/experiments.md S).  So the
    // launch is checked: the workgroups count themselves in (RingDev::arrived), and a kernel not all of whose workgroups have started within
    // 3 ms is closed and launched again with as many workgroups as did start.
    // (chunks carried over from an epoch before -- ring_end_epoch -- are shown to the kernel only once it is known to be whole)
    const unsigned long long carried = r->host->head;
    *reinterpret_cast<volatile unsigned long long *>(&r->host->head) = 0;
    for (int attempt = 0; attempt < 4; ++attempt) {
        // a fresh device-side ring: nothing published, slot 0 holds the call-start history of chunk 0
        mrhip::RingDev init{};
        init.idle_ticks = r->idle_ticks;
        init.opts = static_cast<unsigned long long>(MRHIP_ENV_INT("MRHIP_RING_OPTS", 0));
        init.hist_seq[0] = 1;
        MRHIP_CHECK_HIP(hipMemsetAsync(r->dev, 0, sizeof(mrhip::RingDev), r->stream));
        MRHIP_CHECK_HIP(hipMemcpyAsync(r->dev, &init, offsetof(mrhip::RingDev, chunk_done), hipMemcpyHostToDevice, r->stream));
        MRHIP_CHECK_HIP(hipStreamSynchronize(r->stream));     // (`init` is on this stack)
        r->host->close = 0; r->host->stopped = 0; r->host->arrived = 0; r->host->grid = 0;
        std::atomic_thread_fence(std::memory_order_seq_cst);
        mrhip::PolyArgs a = r->a;
        a.ring_dev = r->dev; a.ring_host = r->host_dev; a.hist = r->hist;
        const char *kname = nullptr;
        const hipError_t e = mrhip::launch_rational_opair(false, a, r->pa, r->block, r->lds, r->stream, &kname, r->f->num_cus, r->f->d_counters);
        if (e != hipSuccess) return fail(MRHIP_ERR_HIP, std::string("launching the ring's resident kernel: ") + hipGetErrorString(e));
        r->f->last_kernel = "rational_opair_kernel";
        // (read from pinned memory, where the feeder copies the count: a device-to-host copy would need a place on the chip this kernel holds)
        // The 3 ms run from the moment the kernel is seen to run at all (its feeder reports the grid): work queued on the device in front of it may
        // keep it waiting for any time (that wait has the deadline of every host-side wait of a ring).
        unsigned long long ag[2] = {0, 0};                   // arrived, grid
        const auto t_launch = std::chrono::steady_clock::now();
        auto t0 = t_launch;
        bool started = false;
        for (;;) {
            ag[0] = *reinterpret_cast<volatile unsigned long long *>(&r->host->arrived);
            ag[1] = *reinterpret_cast<volatile unsigned long long *>(&r->host->grid);
            if (ag[1] != 0 && ag[0] >= ag[1]) break;
            const auto now = std::chrono::steady_clock::now();
            if (ag[1] != 0 && !started) { started = true; t0 = now; }
            if (started && std::chrono::duration<double>(now - t0).count() > 3e-3) break;
            if (!started && std::chrono::duration<double>(now - t_launch).count() > 10.0)
                return fail(MRHIP_ERR_HIP, "the ring's resident kernel did not start within 10 s (internal)");
        }
        if (ag[1] != 0 && ag[0] >= ag[1]) {
            std::atomic_thread_fence(std::memory_order_seq_cst);
            *reinterpret_cast<volatile unsigned long long *>(&r->host->head) = carried;
            r->running = true;
            return MRHIP_OK;
        }
        // not everybody is on the chip: this kernel goes (nothing was published to it), the next one is as large as what did start
        *reinterpret_cast<volatile unsigned long long *>(&r->host->close) = 1;
        MRHIP_CHECK_HIP(hipStreamSynchronize(r->stream));
        if (MRHIP_ENV_INT("MRHIP_DEBUG", 0) != 0) std::fprintf(stderr, "[mrhip] ring: %llu of %llu workgroups started within 3 ms: launching %llu\n", ag[0], ag[1], ag[0]);
        if (ag[0] < 2) return fail(MRHIP_ERR_HIP, "the ring's resident kernel did not start (internal)");
        r->pa.grid_cap = static_cast<int>(ag[0]);
        r->stat_shrunk += 1;
    }
    return fail(MRHIP_ERR_HIP, "the ring's resident kernel does not fit the chip (internal)");
}

// the resident kernel has left (the host closed the ring, or it ended by itself on its idle deadline): chunks it never fetched are
// carried into a new epoch -- history slot, numbering and ticket base re-based -- and, unless the ring is being closed, a new kernel
int ring_end_epoch(mrhip_ring *r, bool relaunch)
{
    MRHIP_CHECK_HIP(hipStreamSynchronize(r->stream));
    r->running = false;
    if (MRHIP_ENV_INT("MRHIP_RING_OPTS", 0) & 256) {       // diagnostics: where the waves' time went (RingDev::stats)
        unsigned long long st[24];
        if (hipMemcpy(st, r->dev->stats, sizeof(st), hipMemcpyDeviceToHost) == hipSuccess && st[3] && st[8])
            std::fprintf(stderr, "[mrhip] ring: compute waves %llu: life %.1f us, barrier %.1f, drain %.1f | loaders %llu: life %.1f us, poll %.1f, stage+prefetch %.1f, "
                                 "barrier %.1f, history %.1f; tiles %llu, flush %llu | feeder: %llu batches, %llu descriptors, %.1f us per batch | idle tiles before a loader's last real tile %llu, last real tile at %.1f..%.1f us, first by %.1f us, real tiles per loader %llu..%llu\n",
                         st[3], st[0] / 100.0 / st[3], st[1] / 100.0 / st[3], st[2] / 100.0 / st[3], st[8], st[4] / 100.0 / st[8], st[5] / 100.0 / st[8],
                         st[6] / 100.0 / st[8], st[7] / 100.0 / st[8], st[11] / 100.0 / st[8], st[9], st[10], st[13], st[15], st[13] ? st[14] / 100.0 / st[13] : 0.0,
                         st[16], ~st[17] / 100.0, st[18] / 100.0, st[19] / 100.0, ~st[20], st[21]);
    }
    if (const char *tp = std::getenv("MRHIP_RING_TRACE"); tp && (MRHIP_ENV_INT("MRHIP_RING_OPTS", 0) & 256)) {
        std::vector<unsigned long long> tr(static_cast<size_t>(mrhip::kRingTraceRows) * 3 * mrhip::kRingTraceTiles);
        if (hipMemcpy(tr.data(), r->dev->trace, tr.size() * 8, hipMemcpyDeviceToHost) == hipSuccess)
            if (FILE *fp = std::fopen(tp, "wb")) { std::fwrite(tr.data(), 8, tr.size(), fp); std::fclose(fp); }
    }
    if (r->host->stopped == 3) {
        if (MRHIP_ENV_INT("MRHIP_DEBUG", 0) != 0) {      // what the kernel left: which history slots were written, which chunks completed
            static mrhip::RingDev snap;
            if (hipMemcpy(&snap, r->dev, sizeof(snap), hipMemcpyDeviceToHost) == hipSuccess) {
                std::fprintf(stderr, "[mrhip] ring gave up: head %llu closed %llu pushed %llu done_upto %llu\n  hist_seq:", snap.head, snap.closed,
                             static_cast<unsigned long long>(r->pushed), static_cast<unsigned long long>(r->done_upto));
                for (int i = 0; i < 32; ++i) std::fprintf(stderr, " %llu", snap.hist_seq[i]);
                std::fprintf(stderr, "\n  gave up: kind %llu (1 a history wait, 2 an impossible descriptor) at chunk %llu, workgroup %llu, its next ticket %llu",
                             snap.stats[12] >> 60, snap.stats[12] & ((1ull << 60) - 1), snap.stats[22] >> 40, snap.stats[22] & ((1ull << 40) - 1));
                std::fprintf(stderr, "\n  host done:");
                for (int i = 0; i < 32; ++i) std::fprintf(stderr, " %llu", r->host->done[i]);
                std::fprintf(stderr, "\n  chunk_done:");
                for (int i = 0; i < 32; ++i) std::fprintf(stderr, " %u", snap.chunk_done[i]);
                std::fprintf(stderr, "\n  tile_base/ngrabs:");
                for (int i = 0; i < 24; ++i) std::fprintf(stderr, " %llu/%u", snap.desc[i].tile_base, snap.desc[i].ngrabs);
                std::fprintf(stderr, "\n");
            }
        }
        return fail(MRHIP_ERR_HIP, "the ring's resident kernel gave up a wait at its deadline (internal)");
    }
    unsigned long long fetched = 0;
    MRHIP_CHECK_HIP(hipMemcpy(&fetched, &r->dev->head, sizeof(fetched), hipMemcpyDeviceToHost));
    // everything fetched has been filtered (the workers leave only when no fetched chunk holds a ticket of theirs)
    const uint64_t left = r->pushed - fetched;
    // (on the ring's own stream, and waited for: a device-to-device hipMemcpy goes down the null stream, which r->stream -- non-blocking -- is
    //  not ordered with, and may return before the copy has run; mrhip_ring_close's copy of slot 0 back into the filter then read a slot 0
    //  that was only partly rewritten: the first 8 KiB pieces new, the rest chunk 0's call-start history)
    if (fetched % mrhip::kRingDepth != 0 && r->slot_bytes) {
        MRHIP_CHECK_HIP(hipMemcpyAsync(r->hist, static_cast<unsigned char *>(r->hist) + (fetched % mrhip::kRingDepth) * r->slot_bytes, r->slot_bytes, hipMemcpyDeviceToDevice, r->stream));
        MRHIP_CHECK_HIP(hipStreamSynchronize(r->stream));
    }
    std::vector<mrhip::RingDesc> keep(static_cast<size_t>(left));
    for (uint64_t i = 0; i < left; ++i) keep[i] = r->host->desc[(fetched + i) % mrhip::kRingDepth];
    const uint64_t tb0 = left ? keep[0].tile_base : r->tile_base;
    for (uint64_t i = 0; i < left; ++i) {
        keep[i].tile_base -= tb0; keep[i].seq = i; keep[i].seq_lo = static_cast<unsigned>(i);
        r->host->desc[i % mrhip::kRingDepth] = keep[i];
    }
    for (int i = 0; i < mrhip::kRingDepth; ++i) r->host->done[i] = 0;
    r->epoch_base += fetched;
    r->pushed = left; r->done_upto = 0; r->tile_base -= tb0;
    std::atomic_thread_fence(std::memory_order_seq_cst);
    r->host->head = left;
    if (fetched > 0 || left > 0) r->stat_restarts += relaunch ? 1 : 0;
    if (relaunch) return ring_launch(r);
    return MRHIP_OK;
}

inline void ring_scan_done(mrhip_ring *r)
{
    while (r->done_upto < r->pushed &&
           reinterpret_cast<volatile unsigned long long *>(r->host->done)[r->done_upto % mrhip::kRingDepth] == r->done_upto + 1ull)
        ++r->done_upto;
}

// every host-side wait has a deadline of its own (far beyond the kernel's): a ring that does not answer is an error, never a hang
struct RingDeadline {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double limit_s;
    explicit RingDeadline(const mrhip_ring *r) : limit_s(10.0 + 4.0 * static_cast<double>(r->idle_ticks) / 1e8) {}
    bool passed() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit_s; }
};

// wait until every chunk below `upto` (this epoch's numbering) is complete
int ring_wait_upto(mrhip_ring *r, uint64_t upto)
{
    int spins = 0;
    const RingDeadline dl(r);
    for (;;) {
        ring_scan_done(r);
        if (r->done_upto >= upto) return MRHIP_OK;
        if (*reinterpret_cast<volatile unsigned long long *>(&r->host->stopped) != 0ull) {
            // the kernel ended under us (idle deadline racing with a push): what it had fetched is complete; carry on in a new epoch
            const uint64_t before = r->epoch_base;
            if (int rc = ring_end_epoch(r, true)) return rc;
            const uint64_t shift = r->epoch_base - before;
            upto = upto > shift ? upto - shift : 0;
            continue;
        }
        if (++spins > 2000) {
            std::this_thread::yield(); spins = 0;
            if (dl.passed()) return fail(MRHIP_ERR_HIP, "the ring did not complete its chunks in time (internal)");
        }
    }
}

}  // namespace

extern "C" {

int mrhip_ring_open(mrhip_filter *f, mrhip_ring **out)
{
    if (!f || !out) return fail(MRHIP_ERR_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (int rc = rates_refused(f, "mrhip_ring_open")) return rc;
    if (f->ring_open) return fail(MRHIP_ERR_INVALID_ARG, "the filter already feeds a ring");
    DeviceGuard guard(f->device);
    if (!guard.ok) return fail(MRHIP_ERR_HIP, "hipSetDevice failed");
    if (int rc = fresh(f)) return rc;
    hipStream_t s_last = f->last_stream_valid ? f->last_stream : f->own_stream;
    if (stream_is_capturing(s_last)) return fail(MRHIP_ERR_UNSUPPORTED, "ring_open while the filter's stream is being captured");
    auto *r = new mrhip_ring();
    r->f = f;
    // (the stream, like the ring's memory below, is taken over from the filter's last ring when there was one: ring_shutdown)
    if (f->ring_cache.stream) { r->stream = f->ring_cache.stream; f->ring_cache.stream = nullptr; }
    else if (hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking) != hipSuccess) { delete r; return fail(MRHIP_ERR_HIP, "hipStreamCreate failed"); }
    auto bail = [&](int rc) { if (r->host) (void)hipHostFree(r->host); if (r->dev) (void)hipFree(r->dev); if (r->hist) (void)hipFree(r->hist);
                              f->last_stream_valid = false;      // (adopt_stream may have made the ring's stream the filter's last: it is gone)
                              (void)hipStreamSynchronize(r->stream); (void)hipStreamDestroy(r->stream); delete r; return rc; };
    if (int rc = adopt_stream(f, r->stream)) return bail(rc);            // behind whatever the filter enqueued before
    const TypeKey tk = type_key(f);
    // the resident kernel: FIRRational / FIRInterpolator shapes the output-pair kernel has a RING instantiation for
    bool resident = (f->kind == MRHIP_FIR_RATIONAL || f->kind == MRHIP_FIR_INTERPOLATOR) && !f->force_generic && !tk.complex_h && !tk.bank &&
                    f->numerics == MRHIP_NUMERICS_STRICT && MRHIP_ENV_INT("MRHIP_RING_RESIDENT", 1) != 0 && f->device >= 0 && f->device < 64;
    if (resident) {
        std::lock_guard<std::mutex> g(g_ring_mutex);
        if (g_resident_rings[f->device] > 0) resident = false;
    }
    if (resident) {
        PolyArgs a{};
        a.taps = f->d_taps;
        a.x_len = 1LL << 24;                          // geometry of a large call: the ring is planned for throughput
        a.n_out = std::max<int64_t>(outputlength_ratio(a.x_len, f->L, f->M, 1), 1);
        a.x_stride = a.x_len; a.y_stride = a.n_out;
        a.u0 = 0; a.d0 = 1; a.zero_start_below = 0;
        a.L = static_cast<int>(f->L); a.M = static_cast<int>(f->M); a.T = static_cast<int>(f->T); a.H = static_cast<int>(f->H);
        a.nch = static_cast<int>(f->nch);
        // (two workgroups per CU: the RING instantiation is built for 128 VGPRs -- at 80 its loader wave worked out of scratch memory and was
        //  the bottleneck; the LDS of the third workgroup goes into larger tiles.  Two pipeline stages only: see DESIGN.md)
        // (Float64 arithmetic: one workgroup per CU is what runs -- two six-wave workgroups do not pack onto the SIMDs, experiments.md S, T -- with
        //  three stages of larger tiles, as the plain kernel is planned there)
        const int ring_wgpc = tk.r_f64 && MRHIP_ENV_INT("MRHIP_RING_F64_WGPC", 1) == 1 ? 1 : 2;
        resident = opair_ring_available(tk, false, a) && plan_rational_opair(tk, false, a, f->num_cus, &r->pa, &r->block, &r->lds, ring_wgpc) &&
                   (r->pa.ns == (ring_wgpc == 1 ? 3 : 2) || MRHIP_ENV_INT("MRHIP_RING_ANY_NS", 0) != 0);
        if (resident) {
            r->a = a;
            // a grab (one ticket, one descriptor look-up) = MRHIP_RING_GRAB_TILES tiles of J steps
            r->pa.steps_per_group = static_cast<unsigned>(std::max(1, MRHIP_ENV_INT("MRHIP_RING_GRAB_TILES", 1))) * static_cast<unsigned>(r->pa.J);
            r->pa.bank_off = -1;                      // the tap columns come straight from global memory (they change with a chunk's u0)
            // tile descriptors of 16 words + a counter per stage; behind them (16-byte aligned) the 2 KiB the loader prefetches chunk descriptors into
            r->lds = ((static_cast<size_t>(r->pa.flags_off) + (4u * 16u + 4u) * static_cast<size_t>(r->pa.ns) + 15u) & ~static_cast<size_t>(15)) + 2048u;
        }
    }
    r->resident = resident;
    {
        int nx = 0;
        r->xccs = hipDeviceGetAttribute(&nx, hipDeviceAttributeNumberOfXccs, f->device) == hipSuccess && nx > 0 ? nx : 0;
    }
    r->phiIdx = f->phiIdx; r->inputDeficit = f->inputDeficit;
    if (resident) {
        r->slot_bytes = static_cast<size_t>(f->nch) * f->H * x_elt(f);
        const int idle_ms = MRHIP_ENV_INT("MRHIP_RING_IDLE_MS", 2000);
        r->idle_ticks = static_cast<uint64_t>(std::max(idle_ms, 1)) * 100000ull;              // 100 MHz
        mrhip_filter::RingCache &rc_ = f->ring_cache;
        if (rc_.host && rc_.slot_bytes == r->slot_bytes) {
            r->host = static_cast<mrhip::RingHost *>(rc_.host); r->host_dev = static_cast<mrhip::RingHost *>(rc_.host_dev);
            r->dev = static_cast<mrhip::RingDev *>(rc_.dev); r->hist = rc_.hist;
            rc_.host = rc_.host_dev = rc_.dev = rc_.hist = nullptr;
        } else if (hipHostMalloc(reinterpret_cast<void **>(&r->host), sizeof(mrhip::RingHost), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
            hipHostGetDevicePointer(reinterpret_cast<void **>(&r->host_dev), r->host, 0) != hipSuccess ||
            hipMalloc(reinterpret_cast<void **>(&r->dev), sizeof(mrhip::RingDev)) != hipSuccess ||
            hipMalloc(&r->hist, std::max<size_t>(r->slot_bytes * mrhip::kRingDepth, 16)) != hipSuccess)
            return bail(fail(MRHIP_ERR_HIP, "allocating the ring failed"));
        std::memset(r->host, 0, sizeof(mrhip::RingHost));
        if (r->slot_bytes && hipMemcpyAsync(r->hist, f->d_hist[f->hist_cur], r->slot_bytes, hipMemcpyDeviceToDevice, r->stream) != hipSuccess)
            return bail(fail(MRHIP_ERR_HIP, "copying the history into the ring failed"));
        {
            std::lock_guard<std::mutex> g(g_ring_mutex);
            if (g_resident_rings[f->device] > 0) return bail(fail(MRHIP_ERR_UNSUPPORTED, "another ring became resident on this device meanwhile: open the ring again"));
            g_resident_rings[f->device] += 1;
        }
        if (int rc = ring_launch(r)) { std::lock_guard<std::mutex> g(g_ring_mutex); g_resident_rings[f->device] -= 1; return bail(rc); }
    } else {
        for (auto &e : r->ev)
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return bail(fail(MRHIP_ERR_HIP, "hipEventCreate failed"));
    }
    f->ring_open = true;
    f->ring = r;
    *out = r;
    return MRHIP_OK;
}

int mrhip_ring_push(mrhip_ring *r, const void *x, int64_t x_len, int64_t x_stride, void *y, int64_t y_capacity, int64_t y_stride,
                    int64_t *n_written, uint64_t *seq)
{
    if (!r) return fail(MRHIP_ERR_INVALID_ARG, "NULL ring");
    if (!r->f) return fail(MRHIP_ERR_INVALID_ARG, "the ring's filter has been destroyed: close the ring");
    mrhip_filter *f = r->f;
    if (n_written) *n_written = 0;
    if (x_len < 0 || y_capacity < 0) return fail(MRHIP_ERR_INVALID_ARG, "negative length");
    if (x_len > 0 && !x) return fail(MRHIP_ERR_INVALID_ARG, "x is NULL");
    if (x_len >= (1LL << 30)) return fail(MRHIP_ERR_INVALID_ARG, "a chunk takes fewer than 2^30 samples per channel");
    if (f->nch > 1 && x_stride < x_len) return fail(MRHIP_ERR_INVALID_ARG, "x_stride < x_len");
    if (!r->resident) {
        DeviceGuard guard(f->device);
        const int slot = static_cast<int>(r->launched % mrhip::kRingDepth);
        if (r->launched >= static_cast<uint64_t>(mrhip::kRingDepth)) MRHIP_CHECK_HIP(hipEventSynchronize(r->ev[slot]));
        f->ring_open = false;                 // (the filter's own entry points refuse calls while it feeds a ring)
        const int rc = filt_device_any(f, x, x_len, x_stride, y, y_capacity, y_stride, n_written, r->stream, false, nullptr);
        f->ring_open = true;
        if (rc) return rc;
        MRHIP_CHECK_HIP(hipEventRecord(r->ev[slot], r->stream));
        if (seq) *seq = r->launched;
        r->ev_seq[slot] = r->launched++;
        return MRHIP_OK;
    }
    const CallPlan p = plan_rational(f->kind, f->L, f->M, r->phiIdx, r->inputDeficit, x_len);
    // reference: error() before any work, Filters.jl:503 (Interpolator), :550 (Rational)
    if (p.n_out > y_capacity) return fail(MRHIP_ERR_BUFFER_TOO_SMALL, "buffer is too small");
    if (p.n_out > 0 && !y) return fail(MRHIP_ERR_INVALID_ARG, "y is NULL");
    if (f->nch > 1 && y_stride < p.n_out) return fail(MRHIP_ERR_INVALID_ARG, "y_stride < output count");
    const int64_t spc = (p.n_out + r->pa.P - 1) / r->pa.P;
    if (spc * f->nch >= (1LL << 31)) return fail(MRHIP_ERR_INVALID_ARG, "chunk too long for the ring");
    DeviceGuard guard(f->device);
    // room: at most depth - 1 chunks in flight, completed IN ORDER below the window (a slot's descriptor and history are
    // recycled only when every older chunk is complete)
    {
        // (MRHIP_RING_INFLIGHT < 63: experiments -- a shallower window tells a latency-bound ring from a rate-bound one)
        const uint64_t window = static_cast<uint64_t>(std::min(std::max(MRHIP_ENV_INT("MRHIP_RING_INFLIGHT", mrhip::kRingDepth - 1), 1), mrhip::kRingDepth - 1));
        if (r->pushed >= window)
            if (int rc = ring_wait_upto(r, r->pushed - (window - 1))) return rc;
    }
    if (*reinterpret_cast<volatile unsigned long long *>(&r->host->stopped) != 0ull)
        if (int rc = ring_end_epoch(r, true)) return rc;                 // the kernel left on its idle deadline: a new one
    mrhip::RingDesc d{};
    d.x = reinterpret_cast<unsigned long long>(x); d.y = reinterpret_cast<unsigned long long>(y);
    d.x_stride = x_stride; d.y_stride = y_stride; d.x_len = x_len; d.n_out = p.n_out;
    d.u0 = p.phi0 - 1; d.d0 = p.d0;
    d.tile_base = r->tile_base;
    d.steps_per_channel = static_cast<unsigned>(std::max<int64_t>(spc, 1));
    d.total_steps = static_cast<unsigned>(spc * f->nch);
    d.ngrabs = std::max(1u, (d.total_steps + r->pa.steps_per_group - 1u) / r->pa.steps_per_group);
    d.spc_magic = step_magic(spc);
    // a chunk of less than MRHIP_RING_FLUSH_MIN_MB (32) of outputs is stored write-through: one L2 write-back per XCD serves every chunk filed
    // so far, but costs the same whatever they hold -- at one channel of 1e6 samples (3.7 MB) more than the write-through stores it saves
    {
        const long long out_bytes = static_cast<long long>(p.n_out) * f->nch * static_cast<long long>(dtype_size(f->ty));
        const long long min_bytes = static_cast<long long>(MRHIP_ENV_INT("MRHIP_RING_FLUSH_MIN_MB", 32)) << 20;
        // The write-back protocol waits for EVERY one of eight XCDs to have written its L2 back (pair_loader.h: ring_flush_duty takes the minimum
        // over flush_done[0..8)), and an XCD's count only moves when one of its workgroups' loader waves wins the duty: on a device that does
        // not show exactly eight XCDs (CPX / DPX / QPX partitions, CU masks), or with a grid so small that an XCD may be left without a
        // workgroup, every chunk completes by write-through stores instead.
        const bool eight = r->xccs == 8 && (r->pa.grid_cap == 0 || r->pa.grid_cap >= 64);
        d.flags = out_bytes < min_bytes || !eight || (MRHIP_ENV_INT("MRHIP_RING_OPTS", 0) & 8192) ? 1u : 0u;
    }
    d.seq = r->pushed; d.seq_lo = static_cast<unsigned>(r->pushed & 0xffffffffull);
    const int slot = static_cast<int>(r->pushed % mrhip::kRingDepth);
    reinterpret_cast<volatile unsigned long long *>(r->host->done)[slot] = 0;
    r->host->desc[slot] = d;
    std::atomic_thread_fence(std::memory_order_release);
    *reinterpret_cast<volatile unsigned long long *>(&r->host->head) = r->pushed + 1;
    if (seq) *seq = r->epoch_base + r->pushed;
    r->pushed += 1;
    r->tile_base += d.ngrabs;
    r->phiIdx = p.phi_end; r->inputDeficit = p.d_end;
    if (n_written) *n_written = p.n_out;
    return MRHIP_OK;
}

int mrhip_ring_push_chunks(mrhip_ring *r, const void *x, int64_t x_len, int64_t x_stride, int64_t chunk, void *y, int64_t y_capacity,
                           int64_t y_stride, int64_t *n_written, uint64_t *last_seq)
{
    if (!r) return fail(MRHIP_ERR_INVALID_ARG, "NULL ring");
    if (!r->f) return fail(MRHIP_ERR_INVALID_ARG, "the ring's filter has been destroyed: close the ring");
    if (n_written) *n_written = 0;
    if (chunk < 1) return fail(MRHIP_ERR_INVALID_ARG, "chunk must be >= 1");
    const mrhip_filter *f = r->f;
    const size_t xelt = dtype_scalar_size(f->tx) * static_cast<size_t>(f->nc), yelt = dtype_size(f->ty);
    int64_t k = 0;
    for (int64_t a0 = 0; a0 < x_len; a0 += chunk) {
        const int64_t len = std::min<int64_t>(chunk, x_len - a0);
        int64_t got = 0;
        const int rc = mrhip_ring_push(r, static_cast<const unsigned char *>(x) + static_cast<size_t>(a0) * xelt, len, x_stride,
                                       static_cast<unsigned char *>(y) + static_cast<size_t>(k) * yelt, y_capacity - k, y_stride, &got, last_seq);
        if (rc) { if (n_written) *n_written = k; return rc; }
        k += got;
    }
    if (n_written) *n_written = k;
    return MRHIP_OK;
}

int mrhip_ring_wait(mrhip_ring *r, uint64_t seq)
{
    if (!r) return fail(MRHIP_ERR_INVALID_ARG, "NULL ring");
    if (!r->f) return fail(MRHIP_ERR_INVALID_ARG, "the ring's filter has been destroyed: close the ring");
    DeviceGuard guard(r->f->device);
    if (!r->resident) {
        if (seq >= r->launched) return fail(MRHIP_ERR_INVALID_ARG, "no such chunk");
        if (seq + mrhip::kRingDepth < r->launched) return MRHIP_OK;        // (its event has been reused: it was waited for then)
        MRHIP_CHECK_HIP(hipEventSynchronize(r->ev[seq % mrhip::kRingDepth]));
        return MRHIP_OK;
    }
    if (seq >= r->epoch_base + r->pushed) return fail(MRHIP_ERR_INVALID_ARG, "no such chunk");
    if (seq < r->epoch_base) return MRHIP_OK;
    // one chunk: its own flag (chunks complete out of order; the in-order cursor only recycles slots)
    uint64_t local = seq - r->epoch_base;
    int spins = 0;
    const RingDeadline dl(r);
    for (;;) {
        if (local < r->done_upto) return MRHIP_OK;
        if (reinterpret_cast<volatile unsigned long long *>(r->host->done)[local % mrhip::kRingDepth] == local + 1ull) return MRHIP_OK;
        if (*reinterpret_cast<volatile unsigned long long *>(&r->host->stopped) != 0ull) {
            const uint64_t before = r->epoch_base;
            if (int rc = ring_end_epoch(r, true)) return rc;
            if (seq < r->epoch_base) return MRHIP_OK;
            local -= r->epoch_base - before;
            continue;
        }
        if (++spins > 2000) {
            std::this_thread::yield(); spins = 0;
            if (dl.passed()) return fail(MRHIP_ERR_HIP, "the ring did not complete the chunk in time (internal)");
        }
    }
}

int mrhip_ring_drain(mrhip_ring *r)
{
    if (!r) return fail(MRHIP_ERR_INVALID_ARG, "NULL ring");
    if (!r->f) return fail(MRHIP_ERR_INVALID_ARG, "the ring's filter has been destroyed: close the ring");
    DeviceGuard guard(r->f->device);
    if (!r->resident) { MRHIP_CHECK_HIP(hipStreamSynchronize(r->stream)); return MRHIP_OK; }
    return ring_wait_upto(r, r->pushed);
}

}  // extern "C"

// Everything mrhip_ring_close does except freeing the handle: the resident kernel leaves, the stream state goes back into the filter, the
// ring's device memory and stream are released.  Also what mrhip_destroy does to a ring its filter still feeds (a garbage collector runs
// the two finalizers in any order): the ring is then an ORPHAN (r->f == NULL) whose entry points fail and whose close only frees it.
int mrhip::ring_shutdown(mrhip_ring *r)
{
    mrhip_filter *f = r->f;
    DeviceGuard guard(f->device);
    int rc = MRHIP_OK;
    if (r->resident) {
        // consume what is published, then leave; a kernel that left earlier on its idle deadline may have missed the last pushes
        for (int round = 0; round < 4 && rc == MRHIP_OK; ++round) {
            *reinterpret_cast<volatile unsigned long long *>(&r->host->close) = 1;
            rc = ring_end_epoch(r, false);
            if (rc || r->pushed == 0) break;
            rc = ring_launch(r);                     // (unfetched chunks: one more short life of the kernel)
        }
        if (rc == MRHIP_OK && r->pushed != 0) rc = fail(MRHIP_ERR_HIP, "the ring could not be drained (internal)");
        if (rc == MRHIP_OK) {
            // the stream goes on in the filter object: state behind the last chunk, its history, the device record
            f->phiIdx = r->phiIdx; f->inputDeficit = r->inputDeficit;
            f->mirror_valid = true;
            hist_leave_zeros(f);
            if (r->slot_bytes && hipMemcpyAsync(f->d_hist[f->hist_cur], r->hist, r->slot_bytes, hipMemcpyDeviceToDevice, r->stream) != hipSuccess)
                rc = fail(MRHIP_ERR_HIP, "copying the history back failed");
            if (rc == MRHIP_OK) rc = rec_push(f, r->stream);
        }
        (void)hipStreamSynchronize(r->stream);
        { std::lock_guard<std::mutex> g(g_ring_mutex); g_resident_rings[f->device] -= 1; }
        // the ring's memory stays with the filter for its next ring (freed by mrhip_destroy: ring_cache_free)
        mrhip_filter::RingCache &rc_ = f->ring_cache;
        if (!rc_.host && r->host && r->dev && r->hist) {
            rc_.host = r->host; rc_.host_dev = r->host_dev; rc_.dev = r->dev; rc_.hist = r->hist; rc_.slot_bytes = r->slot_bytes;
        } else {
            if (r->host) (void)hipHostFree(r->host);
            if (r->dev) (void)hipFree(r->dev);
            if (r->hist) (void)hipFree(r->hist);
        }
        r->host = nullptr; r->host_dev = nullptr; r->dev = nullptr; r->hist = nullptr;
    } else {
        (void)hipStreamSynchronize(r->stream);
        for (auto &e : r->ev) if (e) (void)hipEventDestroy(e);
    }
    // everything the ring enqueued is complete: the filter's next call needs no ordering against the ring's stream
    f->last_stream_valid = false;
    if (!f->ring_cache.stream) f->ring_cache.stream = r->stream;      // (drained above)
    else (void)hipStreamDestroy(r->stream);
    r->stream = nullptr;
    f->ring_open = false;
    f->ring = nullptr;
    r->f = nullptr;
    return rc;
}

void mrhip::ring_cache_free(mrhip_filter *f)
{
    mrhip_filter::RingCache &c = f->ring_cache;
    if (c.host) (void)hipHostFree(c.host);
    if (c.dev) (void)hipFree(c.dev);
    if (c.hist) (void)hipFree(c.hist);
    if (c.stream) (void)hipStreamDestroy(c.stream);
    c = mrhip_filter::RingCache{};
}

extern "C" {

int mrhip_ring_close(mrhip_ring *r)
{
    if (!r) return fail(MRHIP_ERR_INVALID_ARG, "NULL ring");
    const int rc = r->f ? mrhip::ring_shutdown(r) : MRHIP_OK;     // (an orphan: its filter's destruction shut it down)
    delete r;
    return rc;
}

int mrhip_ring_info(const mrhip_ring *r, int64_t *info, int n)
{
    if (!r || !info || n < 0) return fail(MRHIP_ERR_INVALID_ARG, "NULL argument");
    const int64_t v[9] = {r->resident ? 1 : 0, mrhip::kRingDepth, r->resident ? static_cast<int64_t>(r->epoch_base + r->pushed) : static_cast<int64_t>(r->launched),
                          r->stat_restarts, r->resident ? static_cast<int64_t>(r->pa.steps_per_group) : 0, r->resident ? r->pa.P : 0,
                          r->stat_shrunk, r->resident ? static_cast<int64_t>(r->pa.grid_cap) : 0, r->xccs};
    for (int i = 0; i < n && i < 9; ++i) info[i] = v[i];
    return MRHIP_OK;
}

}  // extern "C"
