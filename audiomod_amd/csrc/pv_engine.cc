// pv_engine.cc -- host engine + C ABI (include/audiomod_pv.h) of the MI355X phase-vocoder.
//
// The host stages overlapping STFT frames across channels / blocks / streams and drives the four
// gfx950 kernels of pv_kernels.hip chunk by chunk.  All data-independent decisions (hop sizes,
// per-slice shift increments, output counts, OLA tile geometry) come from the integer planner in
// pv_plan.cc; the device never needs a host round trip inside a chunk.
//
// There is NO CPU fallback: without a gfx950 device every constructor returns PV_ERR_NO_DEVICE.
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstring>
#include <deque>
#include <memory>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "audiomod_pv.h"
#include "pv_kernels.h"
#include "pv_wavefft.h"
#include "pv_plan.h"
#include "pv_carrier.h"
#include "pv_snapshot.h"
#include "pv_whisper.h"

namespace pv {

static thread_local std::string g_last_error;

static int hip_fail(hipError_t e, const char *what, int line) {
    char buf[512];
    snprintf(buf, sizeof buf, "%s failed at pv_engine.cc:%d: %s", what, line, hipGetErrorString(e));
    g_last_error = buf;
    return PV_ERR_HIP;
}
// inside Core::launch_chunk (returns nothing): the first failing call of a launch sequence is remembered with its line
// and reported by the entry point that enqueued it (pv_batch_run / pv_feed)
#define HIPV(call)                                                           \
    do {                                                                     \
        hipError_t e__ = (call);                                             \
        if (e__ != hipSuccess && launch_err == hipSuccess) launch_err = e__, launch_err_line = __LINE__; \
    } while (0)
#define HIPC(call)                                                 \
    do {                                                           \
        hipError_t e__ = (call);                                   \
        if (e__ != hipSuccess) return hip_fail(e__, #call, __LINE__); \
    } while (0)

static int ilog2(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}
static int next_pow2_i(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

static int count_gfx950() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    int ok = 0;
    for (int i = 0; i < n; ++i) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, i) == hipSuccess && strncmp(p.gcnArchName, "gfx950", 6) == 0) ++ok;
    }
    return ok;
}

// The phase stage of a configuration: -1 = none (the modes without a phase recurrence), else its coremode: 0 = the
// propagation kernel, 1 = match kernel + rotation chain, 2 = no phase kernel (synthesis reads the analysis phases)
static int phase_mode(const Derived &d) {
    const bool bypass = d.robotic || d.whisper || d.constant || d.vocoder;
    return bypass ? -1 : ((d.cfg.coremode == 1 || d.cfg.coremode == 2) ? d.cfg.coremode : 0);
}
// LDS bytes of the resampler's filter table: the per-offset float4 rows (Core::tab4) or the sinc table itself
static int res_tab_bytes(const Derived &d) {
    return !d.resample ? 0
           : d.interp  ? d.oversample * (d.filt_len + 1) * 16
                       : (int)((d.sinc.size() * sizeof(float) + 15) & ~(size_t)15);
}

// LDS floats of one staged row of a resampling tile: the stream samples 256 outputs span at the configuration's input
// step, one filter length, and the margins the kernels write past them (Core::init, pool_launch_group, the mixed
// batch's tables: one rule)
static int res_tile_lds_floats(const Derived &d) {
    const double step = d.resample ? (double)d.res_num / (double)d.res_den : 1.0;
    const int tile_span = (int)(kTileOut * step) + (d.resample ? d.filt_len : 0) + 4;
    return (tile_span + 4 + 3) & ~3;
}
// What launch_resample / the uniform pool's resampler reads of a configuration to choose its kernel
static ResArgs res_rung_probe(const Derived &d, int rows, bool fast) {
    ResArgs ra{};
    ra.rows = rows;
    ra.interp = d.interp ? 1 : 0;
    ra.filt_len = d.filt_len;
    ra.oversample = d.oversample;
    ra.lds_floats = res_tile_lds_floats(d);
    ra.tab_bytes = res_tab_bytes(d);
    ra.fast = fast ? 1 : 0;
    return ra;
}
// The refusal of a pitch whose resampling kernel cannot get its LDS: the filter grows with the ratio (make_resampler),
// and so do the table and the tile.  need: the bytes the kernel of this configuration would ask for.
static int refuse_resample_lds(const Derived &d, size_t need, const char *kernel) {
    char msg[384];
    snprintf(msg, sizeof msg,
             "pitch %+.2f semitones is above the limit: its resampling filter has %d taps (rate %d/%d, oversampling %d) and "
             "the %s needs %zu bytes of LDS for table and tile, a workgroup has %d; the fused path resamples up to about "
             "+46 semitones with PV_ARITH_FAST and +56 with PV_ARITH_EXACT",
             (double)d.cfg.pitch_semitones, d.filt_len, d.res_num, d.res_den, d.oversample, kernel, need, 160 * 1024 - 512);
    g_last_error = msg;
    return PV_ERR_UNSUPPORTED;
}

template <typename T> struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    int alloc(size_t count) {
        release();
        n = count;
        HIPC(hipMalloc((void **)&p, (count ? count : 1) * sizeof(T)));
        // Every device buffer starts as zeros (a creation-time cost only).  The kernels read nothing they have not
        // written except slots whose values are provably unused (records and rotations of lanes beyond a step's peak
        // count), but "provably unused" deserves a belt: with this, what such a slot holds cannot depend on what the
        // memory held before -- round 2 saw one bit-identity test fail twice, with identical garbage in one output
        // sample, on what was probably one box of the pool, and never again.
#ifdef PV_POISON // debugging build: NaN / -1 patterns, so that relying on these zeros shows (pv_kernels.hip PV_POISON)
        HIPC(hipMemset(p, 0xFF, (count ? count : 1) * sizeof(T)));
#else
        HIPC(hipMemset(p, 0, (count ? count : 1) * sizeof(T)));
#endif
        return PV_OK;
    }
    // The same with the fill ordered on `st`, for a buffer that only `st`'s work uses: alloc()'s fill is on the default
    // stream, which nothing orders against a non-blocking stream, so work enqueued there right away could be overtaken
    // by it.  (Growing frees the old buffer, which waits for the device.)
    int alloc_on(size_t count, hipStream_t st) {
        release();
        n = count;
        HIPC(hipMalloc((void **)&p, (count ? count : 1) * sizeof(T)));
#ifdef PV_POISON
        HIPC(hipMemsetAsync(p, 0xFF, (count ? count : 1) * sizeof(T), st));
#else
        HIPC(hipMemsetAsync(p, 0, (count ? count : 1) * sizeof(T), st));
#endif
        return PV_OK;
    }
    void swap(DevBuf &o) {
        std::swap(p, o.p);
        std::swap(n, o.n);
    }
    int upload(const std::vector<T> &v) {
        int st = alloc(v.size());
        if (st != PV_OK) return st;
        if (!v.empty()) HIPC(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
        return PV_OK;
    }
};

template <typename T> struct PinBuf {
    T *p = nullptr;
    size_t n = 0;
    ~PinBuf() {
        if (p) (void)hipHostFree(p);
    }
    int alloc(size_t count) {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        n = count;
        HIPC(hipHostMalloc((void **)&p, (count ? count : 1) * sizeof(T), hipHostMallocDefault));
        return PV_OK;
    }
};

// ------------------------------------------------------------------------------------------
// Core: device-resident tables, intermediates and per-stream state for S streams x C channels.
// ------------------------------------------------------------------------------------------
// ------------------------------------------------------------------------------------------
// Host plan of the fused synthesis + overlap-add kernel: for every slice, where its frame lands in the rings,
// the window-sum denominators of the samples it finalises and the resampler's positions for the outputs its wave
// emits.  All of it is data-independent and the same for every row, so it is computed once per slice here
// (64-bit divisions, float window sums in the reference's order) and the kernel only looks things up.
// ------------------------------------------------------------------------------------------
struct ChainBuilder {
    const Derived &d;
    int AR, smask;
    struct Live {
        int64_t P;
        int32_t flags;
    };
    std::deque<Live> live; // frames that may still cover samples not yet finalised, oldest first
    bool any_upper_skip = false;
    int64_t launch_k0 = 0; // first output of the current launch (begin_launch)
    std::vector<ChainSlice> launch_cs; // the current launch's slices, in order (end_launch turns them into run lists)
    std::vector<int64_t> launch_P;
    // the mixed batch's redraw: add() only lays the denominators out (wden_off, wden_count floats so far in the
    // launch); a kernel computes them (pv_kernels.hip pv_mb_build_wden_kernel)
    bool count_only = false;
    int64_t wden_count = 0;

    ChainBuilder(const Derived &dd, int ar, int mask) : d(dd), AR(ar), smask(mask) {}

    static int32_t pmod(int64_t v, int m) {
        int64_t r = v % m;
        return (int32_t)(r < 0 ? r + m : r);
    }
    // window-sum denominator of OLA sample n at the moment writeSlice divides (channelinfo.cc:108 seeds [0] with
    // 1; synthesiseSlice :1073 adds w[i] * float(area * 1.5) per frame, oldest frame first)
    float denominator(int64_t n, bool upper) const {
        float acc = n == 0 ? 1.f : 0.f;
        for (const Live &f : live) {
            if (upper && (f.flags & kSliceUpperChannelsSkip)) continue;
            const int64_t off = n - f.P;
            if (off >= 0 && off < d.N) acc += d.window[(size_t)off] * d.win_gain;
        }
        return acc;
    }
    // out_limit: outputs at or beyond it are not written (the CLI truncates to the input length).
    void add(const SliceRec &r, int64_t out_limit, std::vector<float> &wden, std::vector<float> &wden_hi) {
        ChainSlice c{};
        c.tl = (int32_t)launch_cs.size();
        c.acc_pos = pmod(r.P, AR);
        c.str_pos = (int32_t)(r.P & (int64_t)smask);
        c.adv = r.adv;
        c.flags = r.flags;
        if (r.flags & kSliceUpperChannelsSkip) any_upper_skip = true;
        const int lead = c.acc_pos & 3;
        if (count_only) { // the same layout, nothing computed
            c.wden_off = (int32_t)wden_count;
            wden_count += (r.adv + lead + 3) & ~3;
        } else {
            live.push_back(Live{r.P, r.flags});
            // denominators by ring quads: entry 0 belongs to sample P - (P mod 4); entries outside [P, P + adv) are
            // never used (1.0); every slice starts on a 16-byte boundary
            while (wden.size() & 3) wden.push_back(1.f), wden_hi.push_back(1.f);
            c.wden_off = (int32_t)wden.size();
            for (int i = -lead; i < ((r.adv + lead + 3) & ~3) - lead; ++i) {
                const bool in = i >= 0 && i < r.adv;
                wden.push_back(in ? denominator(r.P + i, false) : 1.f);
                wden_hi.push_back(in && any_upper_skip ? denominator(r.P + i, true) : wden.back());
            }
            const int64_t Pn = r.P + r.adv;
            while (!live.empty() && live.front().P + d.N <= Pn) live.pop_front();
        }
        if (!d.resample) { // the finalised samples are the outputs
            int64_t lo = r.K0, hi = r.K0 + r.cnt;
            if (hi > out_limit) hi = out_limit;
            if (lo > hi) lo = hi;
            c.k_off = (int32_t)(lo - launch_k0);
            c.kcnt = (int32_t)(hi - lo);
        }
        launch_cs.push_back(c);
        launch_P.push_back(r.P);
    }
    // the first output of the launch, relative to which k_off counts
    int64_t begin_launch(const SliceRec &first) {
        launch_k0 = first.K0;
        wden_count = 0;
        launch_cs.clear();
        launch_P.clear();
        return launch_k0;
    }
    // Ends the launch: its slices become the lists of up to `runs_wanted` runs (one workgroup each per row).  Run 0
    // continues from the row's carried accumulator.  A later run starts from an empty one and first re-adds the
    // frames before its range whose tails reach into it -- every frame j with P_j + N > P_start, copied in front of
    // its list with flag bit 1 (rebuilt, not emitted): from its first own sample on, its accumulator then holds the
    // same sums in the same order as the sequential walk.  The number of runs is cut down until that warm-up is at
    // most half a run (and falls back to one run where it would reach before the launch).
    // Appends the lists to `cs` and runs + 1 offsets (relative to the launch's first entry in `cs`) to `run_off`;
    // returns the number of runs.
    int end_launch(int runs_wanted, std::vector<ChainSlice> &cs, std::vector<int32_t> &run_off) {
        const int Tn = (int)launch_cs.size();
        int R = runs_wanted < 1 ? 1 : runs_wanted;
        std::vector<int> start, warm;
        for (; R > 1; R = R / 2) {
            const int L = (Tn + R - 1) / R;
            bool ok = L >= 2;
            start.clear();
            warm.clear();
            for (int r = 1; ok && r < R; ++r) {
                const int a = r * L;
                if (a >= Tn) {
                    ok = false;
                    break;
                }
                int w = a;
                while (w > 0 && launch_P[(size_t)(w - 1)] + d.N > launch_P[(size_t)a]) --w;
                if (w == 0 && launch_P[0] + d.N > launch_P[(size_t)a]) ok = false; // would need frames of the launch before
                if (2 * (a - w) > L) ok = false;
                start.push_back(a);
                warm.push_back(w);
            }
            if (ok) break;
        }
        const size_t base = cs.size();
        if (R <= 1) {
            run_off.push_back(0);
            cs.insert(cs.end(), launch_cs.begin(), launch_cs.end());
            run_off.push_back((int32_t)(cs.size() - base));
            return 1;
        }
        const int L = (Tn + R - 1) / R;
        for (int r = 0; r < R; ++r) {
            run_off.push_back((int32_t)(cs.size() - base));
            const int a = r * L, b = (r + 1) * L < Tn ? (r + 1) * L : Tn;
            if (r > 0)
                for (int j = warm[(size_t)(r - 1)]; j < a; ++j) {
                    ChainSlice w = launch_cs[(size_t)j];
                    w.flags |= 2;
                    cs.push_back(w);
                }
            for (int j = a; j < b; ++j) cs.push_back(launch_cs[(size_t)j]);
        }
        run_off.push_back((int32_t)(cs.size() - base));
        return R;
    }
};

// what one launch of the fused synthesis + overlap-add kernel needs from the host plan
struct ChainLaunch {
    const ChainSlice *slices; // the launch's run lists (device)
    const int32_t *run_off;   // [runs + 1]
    int runs;
    const float *wden, *wden_hi;
    float *out;               // the row-0 address of the launch's first output
    // resampling configurations: the second kernel's tiles for the outputs this launch completes
    const ResTile *res_tiles;
    const uint2 *res_otab;
    int res_ntiles;
    // Batch path: the resampling kernel (arithmetic-bound) runs on its own stream beside what the main stream does
    // next (the following chunk's analysis and match, memory- and latency-bound).  ev_fused: recorded behind this
    // launch's fused kernel; ev_res: recorded behind its resampling; ev_ring_free: the resampling that must have
    // finished before this launch's fused kernel may overwrite the stream ring (two launches back).
    hipStream_t res_stream;
    hipEvent_t ev_fused, ev_res, ev_ring_free;
    bool late_chain; // three-stage order: the rotation chain is handed over by a separate call (part 5)
};

struct Core {
    Derived d;
    int device = 0, S = 0, C = 0, rows = 0;
    int Tc = 0, TR = 0, FR = 0, HP = 0, pkmax = 0, PKP = 0, lookback = 0;
    bool pipelined_planes = false; // set before init() by the batch engine
    int ola_lds_floats = 0;
    int otab_off = 0, wacc_pitch = 0; // layout of one tile's row of host-planned values (pv_kernels.h OlaArgs)
    DevTables tb{};
    DevBuf<int32_t> perm, iperm;
    DevBuf<float2> tw_fwd, tw_inv, st_fwd, st_inv;
    DevBuf<float4> twl_fwd, twl_inv;
    DevBuf<float> window, window_sh, sinc;
    DevBuf<float4> tab4;
    DevBuf<float> mag, phase, outphase, frames, rot;
    DevBuf<float> cmag, cphase; // vocoder: carrier planes [TR][HP]
    DevBuf<uint16_t> peaks;
    DevBuf<int32_t> npk, modes;
    DevBuf<PeakRec> recs;
    // persistent per-row phase state
    DevBuf<float> st_pp, st_po, st_rot;
    DevBuf<int32_t> st_kind;
    // Fused synthesis + overlap-add ("chain", pv_kernels.h ChainArgs): the reference's accumulators live in LDS and
    // their images are carried here between launches.  On by default (AUDIOMOD_PV_FUSED=0 selects the frame ring +
    // tile kernel instead, which cannot represent dropped slices).
    bool use_chain = false;
    // The fused kernel runs one workgroup per (row, run); a batch with fewer than 256 rows splits each row's slices
    // of a launch into runs (ChainBuilder::end_launch) to fill the chip.  Very small batches stay on the tile path
    // (frames through HBM, thousands of small workgroups) unless their plan contains dropped slices (only the fused
    // path's accumulator can represent them) or AUDIOMOD_PV_FUSED=2 asks for it; the streaming engine always takes
    // the fused path (it must follow whatever the caller's call sizes lead to).
    bool chain_required = false; // set before init()
    // (measured, 128 / 64 / 32 rows: fused + runs 31.9 / 20.0 / 12.2 ms per step against the tile path's 31.2 / 17.2 /
    // 12.2 -- below a full chip's worth of rows the rotation chain's serial latency dominates either way, and the
    // tile path's kernels need no warm-up)
    static constexpr int kChainMinRows = 192;
    bool fast_arith = false;  // set before init() by the batch engine (audiomod_pv.h PV_ARITH_FAST); only the fused
                              // wave-FFT path has the fast kernels, everything else computes exactly either way
    bool fuse_phase = false;  // single-stream engine: match kernel and rotation chain in one launch (set by pv_create)
    bool split_analysis = false; // 4096-point frames: the analysis kernel with a frame on two waves (pv_analyze_split_kernel)
    bool ahead = false;       // three-stage order with the analysis one chunk further ahead (pv_batch_run): planes hold three chunks
    bool three_stage = false; // pipelined batch path: resampling of chunk i-2 between the front of i and the fused kernel of i-1
    int chain_AR = 0, chain_smask = 0, chain_waves = 0;
    int chain_max_adv = 0; // set before init(): the largest overlap-add advance the planner can emit
    DevBuf<float> st_acc, stream; // accumulator-ring images (two halves); normalised overlap-add stream rings (resampling only)
    mutable int acc_half = 0;     // which half of st_acc the next fused launch reads
#ifdef PV_DIAG
    static bool debug_stale_acc() {
        static const bool on = [] {
            const char *e = getenv("AUDIOMOD_PV_DEBUG_STALE_ACC");
            return e && atoi(e) != 0;
        }();
        return on;
    }
#endif
    // The formant setting (pv_set_formant / pv_batch_set_formant): the cepstral stage of mode FORMANT_CEPSTRAL as a
    // run-time setting of the plain modes, with its own env_comp.  The stage runs where d.cepstral says so or where the
    // setting is on and moves the envelope at all.
    bool fx_on = false;
    float fx_env_comp = 1.0f;
    bool cepstral_on() const { return d.cepstral || (fx_on && fx_env_comp != 1.0f); }
    float cepstral_env_comp() const { return d.cepstral ? d.env_comp : fx_env_comp; }
    mutable hipError_t launch_err = hipSuccess; // first HIP failure inside launch_chunk since take_launch_error()
    mutable int launch_err_line = 0;
    int take_launch_error() const {
        if (launch_err == hipSuccess) return PV_OK;
        const int rc = hip_fail(launch_err, "a launch / event call of Core::launch_chunk", launch_err_line);
        launch_err = hipSuccess;
        return rc;
    }
    // resample tiles (outputs [ka, kb)) of the fused path
    void build_res_tiles(int64_t ka, int64_t kb, std::vector<ResTile> &tiles, std::vector<uint2> &otab) const;
    static bool chain_wanted() {
        const char *e = getenv("AUDIOMOD_PV_FUSED");
        if (e && atoi(e) == 0) return false;
        const char *sl = getenv("AUDIOMOD_PV_STREAM_LAUNCHES"); // the opt-in one-workgroup streaming kernel chains
        return !(sl && strcmp(sl, "single") == 0);               // the separate stages' device functions
    }
    bool wave_fft() const { return d.fft.nc == 256 || d.fft.nc == 512 || d.fft.nc == 1024 || d.fft.nc == 2048; } // fft 512 ... 4096
    // PV_ARITH_FAST and a free-form fused kernel exists for this configuration (pv_kernels.hip launch_synth_chain):
    // the window-sum denominators are then uploaded as reciprocals
    bool fast_chain() const { return use_chain && fast_capable(); }
    // ... whatever the path: with PV_ARITH_FAST such a configuration ALWAYS takes the fused path (init), so that what
    // an engine computes does not depend on how many rows it was created for -- a batch, its host-staged groups and
    // the single-stream engine run the same kernels and agree bit for bit, as they do under PV_ARITH_EXACT
    bool fast_capable() const { return fast_capable_of(d, fast_arith); }
    // ... for any derived constants (the stream pool asks it per slot)
    static bool fast_capable_of(const Derived &d, bool fast_arith) {
        if (!(fast_arith && (d.fft.nc == 256 || d.fft.nc == 512 || d.fft.nc == 1024 || d.fft.nc == 2048))) return false;
        return synth_chain_has_fast(chain_probe(d));
    }
    // what the fused ladder's predicate (pv_kernels.hip synth_chain_plain_core) reads, from the derived constants alone
    static SynthArgs chain_probe(const Derived &d) {
        SynthArgs probe = synth_variant(d);
        probe.tb.nc = d.fft.nc;
        probe.whisper = d.whisper ? reinterpret_cast<const float *>(&d) : nullptr; // (only tested against null)
        return probe;
    }
    // waves per workgroup the fused kernel of this configuration is compiled for (init sizes chain_waves below it)
    static int chain_wave_bound(const Derived &d, bool fast_arith) {
        return synth_chain_max_waves(chain_probe(d), fast_capable_of(d, fast_arith));
    }
    // what selects the synthesis kernel's variant, from the derived constants alone
    static SynthArgs synth_variant(const Derived &d) {
        SynthArgs sa{};
        sa.do_freq_comp = d.do_freq_comp ? 1 : 0;
        sa.voc_band_len = d.vocoder ? d.voc_band_len : -1;
        sa.robotic = d.robotic ? 1 : 0;
        sa.passthru = d.constant ? 1 : 0;
        sa.coremode = std::max(0, phase_mode(d));
        return sa;
    }
    // The kernels' argument blocks (pv_kernels.h), filled with everything that is a property of this Core: its derived
    // constants, its buffers and its sizes.  nrows: the rows one launch covers -- `rows` on the batch and streaming
    // paths (launch_chunk), C on the slot-table paths, where a launch serves a table of slots with C rows each.  What
    // belongs to one launch (t0, s0, Tn, phase_inc, the input address, the chain's plan and outputs) stays zero here:
    // launch_chunk sets it, the slot-table paths bring it per slot (PoolSlot / PoolParams / MbSlot).
    // A new kernel argument is filled in here, or at the one call site whose value differs.
    AnalyzeArgs analyze_args(int nrows) const;
    MatchArgs match_args(int nrows) const;
    SeqArgs seq_args(int nrows) const;
    PropArgs prop_args(int nrows) const;
    SynthArgs synth_args(int nrows) const;
    ChainArgs chain_args(int nrows) const;
    // the resampling kernel's block in two parts: what every path shares, and on top of it the filter set-up of a Core
    // whose rows all share d (a mixed launch leaves that zero: each slot brings its own through PoolParams)
    ResArgs res_args(int nrows) const;
    ResArgs res_args_uniform(int nrows) const;

    int init(const pv_config &cfg, int dev, int nstreams, int chunk_slices);
    int reset_state(hipStream_t st);
    // tile geometry for outputs [ka, kb) given the slice table (P of slice t = slices[t - t_base].P)
    // The streaming path's single-launch kernel (every mode but the vocoders, wave-FFT sizes).  Measured SLOWER
    // than one launch per stage -- 93 vs 70 us per 480-frame stereo call: the five launches are asynchronous and
    // overlap the kernels, whereas one workgroup runs the stages' latencies back to back on one CU -- so it is
    // opt-in: AUDIOMOD_PV_STREAM_LAUNCHES=single.
    bool can_single_launch() const;
    int build_tiles(const std::vector<SliceRec> &slices, int64_t t_base, int64_t t_end, int64_t ka, int64_t kb,
                    int32_t p_index_base, std::vector<OlaTile> &tiles, std::vector<float> &wacc) const;
    // part: 0 = the whole chunk on `st`; 1 = its front (analysis, match, and the rotation chain handed to
    // st_chain); 2 = its back (synthesis, overlap-add, after waiting for the chain).  Parts 1 and 2 are the two
    // halves of the pipelined phase-locked batch path (pv_batch_run).
    void launch_chunk(const InAddr &ia, int64_t t0, int Tn, const int32_t *d_pinc, const OlaTile *d_tiles,
                      int ntiles, const int64_t *d_P, const float *d_wacc, const float *d_whisper,
                      const InAddr *carrier, float *out, int64_t out_stride_row, int64_t k_base,
                      hipStream_t st, hipEvent_t *ev /* 2*PV_NUM_KERNELS events or null */, int part = 0,
                      hipStream_t st_chain = nullptr /* the chain's own stream (with ev_match / ev_chain) */,
                      hipEvent_t ev_match = nullptr, hipEvent_t ev_chain = nullptr,
                      bool single_launch = false, // single_launch: the streaming path's one-workgroup kernel
                      const struct ChainLaunch *chain = nullptr) const; // non-null: fused synthesis + overlap-add
    // Phase-locked batch path: the rotation chain of chunk i (one workgroup per row, a few waves, pure latency:
    // it leaves 95 % of the chip idle) runs on a second HIP stream while the main stream synthesises and
    // overlap-adds chunk i-1 and analyses and matches chunk i+1.  The slice-indexed planes then hold two chunks.
    // AUDIOMOD_PV_PIPELINE=0 turns it off (one stream, chunk after chunk).
    static bool pipeline_wanted(const pv_config &cfg) {
        const char *e = getenv("AUDIOMOD_PV_PIPELINE");
        if (e && atoi(e) == 0) return false;
        const bool phase_stage = cfg.mode == PV_MODE_NORMAL_SHIFT || cfg.mode == PV_MODE_GENDER_CHANGE ||
                                 cfg.mode == PV_MODE_FORMANT_PRESERVE || cfg.mode == PV_MODE_NORMAL_STRETCH ||
                                 cfg.mode == PV_MODE_FORMANT_CEPSTRAL;
        // coremode 1 only: the coremode-0 kernel streams whole planes and merely trades places with synthesis
        // when it runs beside it (measured: 13.42 vs 13.47 Gsamples/s), coremode 2 has no phase kernel
        // ... and frames up to 2048 points: at 4096 the synthesis waves hold 240 VGPRs, two to a SIMD, and lose
        // more to the chain's waves beside them than the overlap returns (measured: 9.65 vs 9.77 Gsamples/s)
        // (AUDIOMOD_PV_PIPELINE=2 forces it for the larger frames too: for measurements)
        return phase_stage && cfg.coremode == 1 && (cfg.fftsize <= 2048 || (e && atoi(e) == 2));
    }
    bool can_overlap_chain() const { return pipelined_planes; }
};

int Core::init(const pv_config &cfg, int dev, int nstreams, int chunk_slices) {
    int st = derive(cfg, d);
    if (st != PV_OK) return st;
    if (d.N > 8192) {
        g_last_error = "fftsize above 8192 is not supported by the phase kernel";
        return PV_ERR_UNSUPPORTED;
    }
    S = nstreams;
    C = cfg.channels;
    rows = S * C;
    if (rows > 65535) { // several kernels put the rows on grid.y
        g_last_error = "more than 65535 rows (streams x channels) in one batch: split it";
        return PV_ERR_UNSUPPORTED;
    }
    HP = d.hs + 8; // row pitch of the mag / phase planes (16-byte aligned rows)
    pkmax = d.hs / 3 + 2;
    PKP = (pkmax + 7) & ~7;
    // frames that can overlap one OLA tile / that must stay in the ring behind the newest slice
    const double step = d.resample ? (double)d.res_num / (double)d.res_den : 1.0;
    const int tile_span = (int)(kTileOut * step) + (d.resample ? d.filt_len : 0) + 4;
    ola_lds_floats = res_tile_lds_floats(d); // a multiple of 4: the gather writes the tile four samples at a time
    otab_off = (ola_lds_floats + 3) & ~3;
    wacc_pitch = otab_off + 2 * kTileOut;
    lookback = (d.N + tile_span) / d.min_shift + 3;
    use_chain = chain_wanted() && (chain_required || rows >= kChainMinRows || fast_capable());
    if (const char *e = getenv("AUDIOMOD_PV_FUSED")) // =2: the fused path whatever the row count
        if (atoi(e) == 2) use_chain = true;
    if (!use_chain && (tile_span + d.N) / d.min_shift + 3 > kMaxTileFrames) {
        if (chain_wanted()) use_chain = true; // the tile path cannot hold that many frames per tile: fused after all
    }
    if (!use_chain && (tile_span + d.N) / d.min_shift + 3 > kMaxTileFrames) {
        g_last_error = "hop too small relative to the FFT size for the OLA tile";
        return PV_ERR_UNSUPPORTED;
    }
    // the resampling kernel of this configuration must get its LDS: decided from the derived constants, before any
    // device call (the mixed pool and the mixed batch check their ranges the same way)
    if (d.resample) {
        if (use_chain) {
            const ResRung rr = resample_rung(res_rung_probe(d, rows, fast_chain()));
            if (!rr.fits) return refuse_resample_lds(d, rr.lds_bytes, "resampling kernel");
        } else {
            OlaArgs probe{};
            probe.tab_bytes = res_tab_bytes(d);
            probe.lds_floats = ola_lds_floats;
            if (ola_lds_bytes(probe, 2) > 160 * 1024 - 512)
                return refuse_resample_lds(d, ola_lds_bytes(probe, 2), "overlap-add and resampling kernel");
        }
    }
    if (count_gfx950() <= 0) {
        g_last_error = "no gfx950 (MI355X) device visible: this library has no CPU fallback";
        return PV_ERR_NO_DEVICE;
    }
    device = dev;
    HIPC(hipSetDevice(dev));
    {
        hipDeviceProp_t p;
        HIPC(hipGetDeviceProperties(&p, dev));
        if (strncmp(p.gcnArchName, "gfx950", 6) != 0) {
            g_last_error = std::string("device is ") + p.gcnArchName + ", kernels are built for gfx950 only";
            return PV_ERR_NO_DEVICE;
        }
    }
    if (!lds_starts_at_zero()) {
        g_last_error = "internal: an analysis kernel was built with static LDS (its atan2f table address assumes none)";
        return PV_ERR_HIP;
    }
    if (use_chain) {
        // ring sizes and waves per workgroup of the chain kernel: as many waves (slices of a row in flight) as LDS
        // holds.  While a wave resamples slice t the others may finalise up to slice t + W - 1, and whole blocks of
        // 64 outputs are deferred by up to one slice (ChainBuilder), so the stream ring keeps W advances plus one
        // filter length plus the span of 64 outputs.
        if (chain_max_adv <= 0) {
            const bool fixed_shift = phase_mode(d) < 0;
            double m = fixed_shift ? (double)d.hop : (d.int_ratio ? (double)d.hop * d.hs_ratio : 2.0 * d.hop * d.hs_ratio + 1);
            chain_max_adv = (int)(m < d.N ? m + 1 : d.N);
        }
        chain_AR = d.N + 4;
        // (beside the rotation chain's kernel -- the pipelined batch path -- twelve: its six-wave workgroups then
        // find a CU's fourth wave slot and 8 KB of LDS free and run at their stand-alone speed; with fourteen or
        // sixteen they wait for a fused workgroup to finish and the overlap is gone: 54.1 vs 58.6 ms per step)
        {
            const char *e3 = getenv("AUDIOMOD_PV_THREE_STAGE");
            three_stage = pipelined_planes && d.resample && !(e3 && atoi(e3) == 0);
        }
        // ... and no more than the kernel the ladder picks is compiled for: eight at fft 4096, twelve for the all-modes
        // variant and the reference-order formant / gender kernel, else sixteen (pv_kernels.hip chain_kernel_max_threads;
        // the rule is stated there, once, beside the predicate)
        const int wmax_rung = chain_wave_bound(d, fast_arith);
        int wmax = (pipelined_planes && !three_stage) ? 12 : 16;
        if (wmax > wmax_rung) wmax = wmax_rung;
        if (const char *e = getenv("AUDIOMOD_PV_CHAIN_WAVES")) { // tuning knob: upper bound of waves per workgroup
            const int v = atoi(e);
            if (v >= 1 && v <= (d.fft.nc == 2048 ? 8 : 16)) wmax = v;
        }
        ChainArgs probe{};
        probe.AR = chain_AR;
        chain_waves = 0;
        for (int w = wmax; w >= 1; --w) {
            probe.waves = w;
            if (chain_lds_bytes(probe, wave_fft() ? d.fft.nc : 0) <= 160 * 1024 - 512) {
                chain_waves = w;
                break;
            }
        }
        if (chain_waves == 0) {
            g_last_error = "the overlap-add ring of this configuration does not fit the LDS";
            return PV_ERR_UNSUPPORTED;
        }
        // the stream ring keeps what one launch finalises plus the history the next launch's first windows reach
        // back into (one filter length), with room to spare
        chain_smask = next_pow2_i(2 * chunk_slices * chain_max_adv + 4 * d.N + 1024) - 1;
    }
    Tc = chunk_slices;
    // slice-indexed planes keep the last slice of the previous launch (pv_kernels.h); the pipelined batch path
    // has two chunks in flight (the front of chunk i+1 runs before the back of chunk i)
    {
        // Round 3: with the free-form resampling kernel the rotation chain of chunk i (0.3-0.4 ms beside it) outlasts
        // the resampling of chunk i-2 (0.28 ms) and delays the fused kernel, whose workgroups need whole CUs.  The
        // analysis of chunk i+1 therefore moves in between -- M(i) -> chain(i) | R(i-2), A(i+1), F(i-1) -- which needs
        // the planes of three chunks.  AUDIOMOD_PV_AHEAD=0: round 2's order.
        const char *ea = getenv("AUDIOMOD_PV_AHEAD"), *er = getenv("AUDIOMOD_PV_RES_STREAM");
        ahead = use_chain && three_stage && wave_fft() && !(ea && atoi(ea) == 0) && !(er && atoi(er) != 0);
    }
    TR = (nstreams > 0 && pipelined_planes) ? (ahead ? 3 : 2) * Tc + 1 : Tc + 1;
    FR = next_pow2_i(Tc + lookback + 1);

    // tables
    std::vector<int32_t> ip(d.fft.nc);
    for (int j = 0; j < d.fft.nc; ++j) ip[d.fft.perm[j]] = j;
    if ((st = perm.upload(d.fft.perm)) != PV_OK) return st;
    if ((st = iperm.upload(ip)) != PV_OK) return st;
    auto up2 = [&](DevBuf<float2> &b, const std::vector<cpx> &v) -> int {
        std::vector<float2> t(v.size());
        for (size_t i = 0; i < v.size(); ++i) t[i] = make_float2(v[i].r, v[i].i);
        return b.upload(t);
    };
    if ((st = up2(tw_fwd, d.fft.tw_fwd)) != PV_OK) return st;
    if ((st = up2(tw_inv, d.fft.tw_inv)) != PV_OK) return st;
    if ((st = up2(st_fwd, d.fft.st_fwd)) != PV_OK) return st;
    if (wave_fft()) { // lane-major twiddle tables of the wave-per-frame kernels
        auto lane_table = [&](const std::vector<cpx> &tw, DevBuf<float4> &dst) -> int {
            std::vector<cf> twc(tw.size());
            for (size_t i = 0; i < tw.size(); ++i) twc[i] = cf{tw[i].r, tw[i].i};
            const int entries = d.fft.nc == 256    ? wf_lane_table_entries<WF<256>>()
                                : d.fft.nc == 512  ? wf_lane_table_entries<WF<512>>()
                                : d.fft.nc == 1024 ? wf_lane_table_entries<WF<1024>>()
                                                   : wf_lane_table_entries<WF<2048>>();
            std::vector<cf> out(2 * (size_t)entries * 64);
            if (d.fft.nc == 256) wf_build_lane_table<WF<256>>(twc.data(), out.data());
            else if (d.fft.nc == 512) wf_build_lane_table<WF<512>>(twc.data(), out.data());
            else if (d.fft.nc == 1024) wf_build_lane_table<WF<1024>>(twc.data(), out.data());
            else wf_build_lane_table<WF<2048>>(twc.data(), out.data());
            std::vector<float4> o4((size_t)entries * 64);
            for (size_t i = 0; i < o4.size(); ++i) o4[i] = make_float4(out[2 * i].x, out[2 * i].y, out[2 * i + 1].x, out[2 * i + 1].y);
            return dst.upload(o4);
        };
        {
            // AUDIOMOD_PV_SPLIT_ANALYSIS=0: the one-wave kernel (also what the opt-in one-workgroup streaming kernel calls)
            const char *es = getenv("AUDIOMOD_PV_SPLIT_ANALYSIS");
            const char *sl = getenv("AUDIOMOD_PV_STREAM_LAUNCHES");
            split_analysis = d.fft.nc == 2048 && !(es && atoi(es) == 0) && !(sl && strcmp(sl, "single") == 0);
        }
        if (split_analysis) {
            std::vector<cf> twc(d.fft.tw_fwd.size());
            for (size_t i = 0; i < twc.size(); ++i) twc[i] = cf{d.fft.tw_fwd[i].r, d.fft.tw_fwd[i].i};
            const int entries = wf_lane_table_entries<WF2048S>();
            std::vector<cf> out(2 * (size_t)entries * WF2048S::LANES);
            wf_build_lane_table<WF2048S>(twc.data(), out.data());
            std::vector<float4> o4((size_t)entries * WF2048S::LANES);
            for (size_t i = 0; i < o4.size(); ++i) o4[i] = make_float4(out[2 * i].x, out[2 * i].y, out[2 * i + 1].x, out[2 * i + 1].y);
            if ((st = twl_fwd.upload(o4)) != PV_OK) return st;
        } else if ((st = lane_table(d.fft.tw_fwd, twl_fwd)) != PV_OK) return st;
        if ((st = lane_table(d.fft.tw_inv, twl_inv)) != PV_OK) return st;
    }
    if ((st = up2(st_inv, d.fft.st_inv)) != PV_OK) return st;
    if ((st = window.upload(d.window)) != PV_OK) return st;
    {
        // the window delayed by d = 0..3 samples: a frame that starts d floats past a 16-byte boundary is read
        // in aligned 16-byte pieces and multiplied by the copy that lines up with it (pv_analyze_wave_kernel)
        const size_t pitch = (size_t)d.N + 8;
        std::vector<float> sh(4 * pitch, 0.f);
        for (int dd = 0; dd < 4; ++dd)
            for (int j = 0; j < d.N; ++j) sh[dd * pitch + j + dd] = d.window[j];
        if ((st = window_sh.upload(sh)) != PV_OK) return st;
    }
    if ((st = sinc.upload(d.sinc)) != PV_OK) return st;
    {
        // interpolated-sinc coefficients expanded per sub-sample offset: row `off`, tap j = the four table
        // entries sinc[4 + (j+1)*ov - off + {-2,-1,0,1}] that resampler_basic_interpolate_single multiplies
        // into its four accumulators (resample.c:494-535); rows padded to filt_len + 1 (LDS bank spread)
        std::vector<float4> t4;
        if (d.resample && d.interp) {
            t4.assign((size_t)d.oversample * (d.filt_len + 1), make_float4(0, 0, 0, 0));
            for (int off = 0; off < d.oversample; ++off)
                for (int j = 0; j < d.filt_len; ++j) {
                    const float *sp = d.sinc.data() + 4 + (j + 1) * d.oversample - off - 2;
                    t4[(size_t)off * (d.filt_len + 1) + j] = make_float4(sp[0], sp[1], sp[2], sp[3]);
                }
        }
        if ((st = tab4.upload(t4)) != PV_OK) return st;
    }

    tb.N = d.N;
    tb.hs = d.hs;
    tb.H = d.H;
    tb.HP = HP;
    tb.nc = d.fft.nc;
    tb.log2nc = ilog2(d.fft.nc);
    tb.nstages = d.fft.nstages;
    for (int s = 0; s < d.fft.nstages; ++s) {
        tb.radix[s] = d.fft.radix[s];
        tb.log2m[s] = ilog2(d.fft.m[s]);
        tb.fstride[s] = d.fft.fstride[s];
    }
    tb.perm = perm.p;
    tb.iperm = iperm.p;
    tb.tw_fwd = tw_fwd.p;
    tb.twl_fwd = twl_fwd.p;
    tb.twl_inv = twl_inv.p;
    tb.tw_inv = tw_inv.p;
    tb.st_fwd = st_fwd.p;
    tb.st_inv = st_inv.p;
    tb.window = window.p;
    tb.window_sh = window_sh.p;

    const int cm = d.cfg.coremode;
    const size_t planes = (size_t)rows * TR;
    if ((st = mag.alloc(planes * HP)) != PV_OK) return st;
    if ((st = phase.alloc(planes * HP)) != PV_OK) return st;
    if (use_chain) FR = next_pow2_i(Tc + 1); // the chain reads a launch's own frames only (and none at wave-FFT sizes)
    if (!(use_chain && wave_fft()))
        if ((st = frames.alloc((size_t)rows * FR * d.N)) != PV_OK) return st;
    if (use_chain) {
        if ((st = st_acc.alloc(2 * (size_t)rows * chain_AR)) != PV_OK) return st; // read half + written half, swapped per launch
        if (d.resample)
            if ((st = stream.alloc((size_t)rows * ((size_t)chain_smask + 1))) != PV_OK) return st;
    }
    const bool bypass = phase_mode(d) < 0; // modes without a phase recurrence
    if (d.vocoder) {
        if ((st = cmag.alloc((size_t)TR * HP)) != PV_OK) return st;
        if ((st = cphase.alloc((size_t)TR * HP)) != PV_OK) return st;
    }
    if (!bypass && cm != 2) {
        if ((st = outphase.alloc(planes * HP)) != PV_OK) return st;
        if ((st = st_po.alloc((size_t)rows * d.hs)) != PV_OK) return st;
        if ((st = st_pp.alloc((size_t)rows * d.hs)) != PV_OK) return st;
    }
    if (!bypass && cm == 1) {
        if ((st = peaks.alloc(planes * PKP)) != PV_OK) return st;
        if ((st = npk.alloc(planes)) != PV_OK) return st;
        if ((st = modes.alloc(planes)) != PV_OK) return st;
        if ((st = recs.alloc(planes * PKP)) != PV_OK) return st;
        if ((st = rot.alloc(planes * PKP)) != PV_OK) return st;
        if ((st = st_rot.alloc((size_t)rows * PKP)) != PV_OK) return st;
        if ((st = st_kind.alloc((size_t)rows)) != PV_OK) return st;
    }
    return reset_state(nullptr);
}

int Core::reset_state(hipStream_t st) {
    if (st_pp.p) HIPC(hipMemsetAsync(st_pp.p, 0, st_pp.n * sizeof(float), st));
    if (st_po.p) HIPC(hipMemsetAsync(st_po.p, 0, st_po.n * sizeof(float), st));
    if (st_kind.p) HIPC(hipMemsetAsync(st_kind.p, 0, st_kind.n * sizeof(int32_t), st));
#ifdef PV_DIAG
    if (debug_stale_acc()) return PV_OK;
#endif
    if (st_acc.p) HIPC(hipMemsetAsync(st_acc.p, 0, st_acc.n * sizeof(float), st));
    acc_half = 0;
    return PV_OK;
}

bool Core::can_single_launch() const {
    static const bool on = [] {
        const char *e = getenv("AUDIOMOD_PV_STREAM_LAUNCHES");
        return e && strcmp(e, "single") == 0;
    }();
    if (!on || d.vocoder || use_chain) return false;
    StreamArgs probe{};
    probe.aa.tb = tb;
    probe.ma.hs = d.hs;
    probe.ma.PKP = PKP;
    probe.qa.hs = d.hs;
    probe.qa.PKP = PKP;
    probe.coremode = 1;
    probe.oa.tab_bytes = res_tab_bytes(d);
    probe.oa.lds_floats = ola_lds_floats;
    return stream_kernel_supported(probe);
}

int Core::build_tiles(const std::vector<SliceRec> &slices, int64_t t_base, int64_t t_end, int64_t ka, int64_t kb,
                      int32_t p_index_base, std::vector<OlaTile> &tiles, std::vector<float> &wacc) const {
    // slices[t - t_base] must exist for every t in [max(t_base, t_end - FR), t_end); a tile that needed an
    // older frame would be rejected below anyway (the frame ring no longer holds it)
    int64_t t_lo = t_end - FR > t_base ? t_end - FR : t_base; // monotone cursors
    int64_t t_hi = t_lo;
    for (int64_t k0 = ka; k0 < kb; k0 += kTileOut) {
        OlaTile tl{};
        tl.k0 = k0;
        tl.kcnt = (int32_t)((kb - k0) < kTileOut ? (kb - k0) : kTileOut);
        int64_t n_lo, n_hi;
        if (d.resample) {
            auto pos = [&](int64_t k) {
                return (int64_t)(d.filt_len / 2) + (int64_t)(((unsigned __int128)k * d.res_num) / d.res_den);
            };
            n_lo = pos(k0) - d.filt_len + 1;
            n_hi = pos(k0 + tl.kcnt - 1);
        } else {
            n_lo = k0;
            n_hi = k0 + tl.kcnt - 1;
        }
        tl.n_lo = n_lo;
        tl.n_cnt = (int32_t)(n_hi - n_lo + 1);
        if (tl.n_cnt > ola_lds_floats) {
            g_last_error = "internal: OLA tile larger than its LDS budget";
            return PV_ERR_UNSUPPORTED;
        }
        const int64_t n0 = n_lo < 0 ? 0 : n_lo;
        // t_first: smallest t with P_t + N > n0 ; t_last: largest t (< t_end) with P_t <= n_hi
        while (t_lo < t_end && slices[(size_t)(t_lo - t_base)].P + d.N <= n0) ++t_lo;
        if (t_hi < t_lo) t_hi = t_lo;
        while (t_hi + 1 < t_end && slices[(size_t)(t_hi + 1 - t_base)].P <= n_hi) ++t_hi;
        if (t_lo > t_base && t_lo == t_end - FR && slices[(size_t)(t_lo - 1 - t_base)].P + d.N > n0) {
            g_last_error = "internal: OLA tile needs a frame the ring no longer holds";
            return PV_ERR_UNSUPPORTED;
        }
        if (t_lo >= t_end) {
            g_last_error = "internal: OLA tile has no covering slice";
            return PV_ERR_UNSUPPORTED;
        }
        tl.t_first = (int32_t)t_lo;
        tl.t_cnt = (int32_t)(t_hi - t_lo + 1);
        if (tl.t_cnt > kMaxTileFrames || t_end - t_lo > FR) {
            g_last_error = "internal: OLA tile overlaps too many frames";
            return PV_ERR_UNSUPPORTED;
        }
        tl.p_off = (int32_t)(t_lo - p_index_base);
        tiles.push_back(tl);
        // window-sum denominator of every OLA sample of the tile: windowAccumulator at the moment writeSlice
        // divides (channelinfo.cc:108 seeds [0] with 1; synthesiseSlice :1073 adds w[i] * float(area*1.5) per
        // frame, ascending t).  Float arithmetic, evaluated exactly as written (-ffp-contract=off).
        const size_t wbase = wacc.size();
        wacc.resize(wbase + (size_t)wacc_pitch, 1.0f);
        for (int i = 0; i < tl.n_cnt; ++i) {
            const int64_t n = n_lo + i;
            float acc = n == 0 ? 1.f : 0.f;
            for (int64_t t = t_lo; t <= t_hi; ++t) {
                const int64_t off = n - slices[(size_t)(t - t_base)].P;
                if (off >= 0 && off < d.N) acc += d.window[(size_t)off] * d.win_gain;
            }
            wacc[wbase + (size_t)i] = acc;
        }
        // where each output of the tile sits in the OLA stream: last_sample = filt_len/2 + floor(k*num/den),
        // samp_frac_num = (k*num) mod den (closed form of resample.c:548-554 from skip_zeros :1225), and from
        // those the sub-sample offset and the interpolation fraction of resampler_basic_interpolate_single
        // (:494-500, float arithmetic as written there).  Data-independent and the same for every row, so the
        // 64-bit divisions happen here once instead of once per row in the kernel.
        if (d.resample) {
            uint32_t *ot = reinterpret_cast<uint32_t *>(wacc.data() + wbase + (size_t)otab_off);
            for (int o = 0; o < tl.kcnt; ++o) {
                const unsigned __int128 tot = (unsigned __int128)(k0 + o) * d.res_num;
                const int64_t pos = (int64_t)(d.filt_len / 2) + (int64_t)(tot / d.res_den);
                const uint32_t frac_num = (uint32_t)(tot % d.res_den);
                const uint32_t xoff = (uint32_t)(pos - d.filt_len + 1 - n_lo);
                uint32_t sub, fbits = 0;
                if (d.interp) {
                    const uint32_t ov = (uint32_t)d.oversample;
                    sub = frac_num * ov / d.res_den;
                    const float frac = ((float)((frac_num * ov) % d.res_den)) / d.res_den;
                    memcpy(&fbits, &frac, 4);
                } else {
                    sub = frac_num;
                }
                ot[2 * o] = xoff | (sub << 16);
                ot[2 * o + 1] = fbits;
            }
        }
    }
    return PV_OK;
}

// (the stream pool calls it with each slot's own constants)
static void build_res_tiles_of(const Derived &d, int64_t ka, int64_t kb, std::vector<ResTile> &tiles, std::vector<uint2> &otab,
                               bool tiles_only = false);
void Core::build_res_tiles(int64_t ka, int64_t kb, std::vector<ResTile> &tiles, std::vector<uint2> &otab) const {
    build_res_tiles_of(d, ka, kb, tiles, otab);
}
// tiles_only: the tile headers alone (the mixed batch's redraw: pv_mb_build_otab_kernel writes the table)
static void build_res_tiles_of(const Derived &d, int64_t ka, int64_t kb, std::vector<ResTile> &tiles, std::vector<uint2> &otab,
                               bool tiles_only) {
    for (int64_t k0 = ka; k0 < kb; k0 += kTileOut) {
        ResTile tl{};
        tl.k0 = k0;
        tl.kcnt = (int32_t)((kb - k0) < kTileOut ? (kb - k0) : kTileOut);
        auto pos = [&](int64_t k) {
            return (int64_t)(d.filt_len / 2) + (int64_t)(((unsigned __int128)k * d.res_num) / d.res_den);
        };
        tl.n_lo = pos(k0) - d.filt_len + 1;
        tl.n_cnt = (int32_t)(pos(k0 + tl.kcnt - 1) - tl.n_lo + 1);
        tiles.push_back(tl);
        if (tiles_only) continue;
        // where each output of the tile sits in the stream: last_sample = filt_len/2 + floor(k*num/den),
        // samp_frac_num = (k*num) mod den (closed form of resample.c:548-554 from skip_zeros :1225), and from those
        // the sub-sample offset and the interpolation fraction of resampler_basic_interpolate_single (:494-500)
        for (int o = 0; o < kTileOut; ++o) {
            if (o >= tl.kcnt) {
                otab.push_back(make_uint2(0u, 0u));
                continue;
            }
            const unsigned __int128 tot = (unsigned __int128)(k0 + o) * d.res_num;
            const int64_t p = (int64_t)(d.filt_len / 2) + (int64_t)(tot / d.res_den);
            const uint32_t frac_num = (uint32_t)(tot % d.res_den);
            const uint32_t xoff = (uint32_t)(p - d.filt_len + 1 - tl.n_lo);
            uint32_t sub, fbits = 0;
            if (d.interp) {
                const uint32_t ov = (uint32_t)d.oversample;
                sub = frac_num * ov / d.res_den;
                const float frac = ((float)((frac_num * ov) % d.res_den)) / d.res_den;
                memcpy(&fbits, &frac, 4);
            } else {
                sub = frac_num;
            }
            otab.push_back(make_uint2(xoff | (sub << 16), fbits));
        }
    }
}

AnalyzeArgs Core::analyze_args(int nrows) const {
    AnalyzeArgs aa{};
    aa.tb = tb;
    aa.hop = d.hop;
    aa.TR = TR;
    aa.rows = nrows;
    aa.PKP = PKP;
    aa.find_peaks = phase_mode(d) == 1 ? 1 : 0;
    aa.split = split_analysis ? 1 : 0;
    aa.mag = mag.p;
    aa.phase = phase.p;
    aa.peaks = peaks.p;
    aa.npk = npk.p;
    return aa;
}
MatchArgs Core::match_args(int nrows) const {
    MatchArgs ma{};
    ma.N = d.N, ma.hs = d.hs, ma.HP = HP, ma.PKP = PKP, ma.C = C, ma.hop = d.hop, ma.TR = TR, ma.rows = nrows;
    ma.two_pi_hop = d.two_pi_hop;
    ma.phase = phase.p, ma.peaks = peaks.p, ma.npk = npk.p, ma.recs = recs.p, ma.modes = modes.p;
    return ma;
}
SeqArgs Core::seq_args(int nrows) const {
    SeqArgs qa{};
    qa.N = d.N, qa.hs = d.hs, qa.HP = HP, qa.PKP = PKP, qa.C = C, qa.hop = d.hop, qa.TR = TR, qa.rows = nrows;
    qa.two_pi_hop = d.two_pi_hop;
    qa.phase = phase.p, qa.peaks = peaks.p, qa.npk = npk.p, qa.recs = recs.p, qa.modes = modes.p;
    qa.rot = rot.p, qa.outphase = outphase.p;
    qa.st_kind = st_kind.p, qa.st_rot = st_rot.p, qa.st_po = st_po.p;
    qa.high_prio = 1, qa.narrow = 0; // (launch_chunk alone reads the environment's knobs for these)
    return qa;
}
PropArgs Core::prop_args(int nrows) const {
    PropArgs pa{};
    pa.N = d.N, pa.hs = d.hs, pa.HP = HP, pa.C = C, pa.hop = d.hop, pa.TR = TR, pa.rows = nrows;
    pa.two_pi_hop = d.two_pi_hop;
    pa.phase = phase.p, pa.outphase = outphase.p, pa.st_pp = st_pp.p, pa.st_po = st_po.p;
    return pa;
}
SynthArgs Core::synth_args(int nrows) const {
    // passthru, voc_band_len and the carrier planes come from d on every path: pool_scope and mb_scope refuse the
    // CONSTANT and vocoder modes (and WHISPER), so on the slot-table paths they are 0, -1 and null as before.  Only
    // `whisper` is missing: the random phases are a launch's (launch_chunk).
    SynthArgs sa = synth_variant(d);
    sa.tb = tb;
    sa.hop = d.hop;
    sa.C = C;
    sa.two_pi_hop = d.two_pi_hop;
    sa.freq_comp = d.freq_comp;
    sa.fixed_gain = d.fixed_gain;
    sa.inv_n = d.inv_n;
    sa.cmag = cmag.p;
    sa.cphase = cphase.p;
    sa.TR = TR;
    sa.rows = nrows;
    sa.PKP = PKP;
    sa.mag = mag.p, sa.phase = phase.p, sa.outphase = outphase.p, sa.peaks = peaks.p, sa.npk = npk.p;
    sa.modes = modes.p, sa.rot = rot.p, sa.frames = frames.p, sa.FR = FR;
    return sa;
}
ChainArgs Core::chain_args(int nrows) const {
    ChainArgs ca{};
    ca.N = d.N;
    ca.rows = nrows;
    ca.C = C;
    ca.AR = chain_AR;
    ca.smask = chain_smask;
    ca.waves = chain_waves;
    ca.runs = 1; // (launch_chunk: the launch's own; the mixed batch: per slot, MbSlot)
    ca.st_acc = st_acc.p;
    ca.stream = stream.p;
    ca.resample = d.resample ? 1 : 0;
    ca.frames = frames.p;
    ca.FR = FR;
    ca.fast = fast_chain() ? 1 : 0;
    return ca;
}
ResArgs Core::res_args(int nrows) const {
    ResArgs ra{};
    ra.rows = nrows;
    ra.smask = chain_smask;
    ra.stream = stream.p;
    return ra;
}
ResArgs Core::res_args_uniform(int nrows) const {
    ResArgs ra = res_args(nrows);
    ra.interp = d.interp ? 1 : 0;
    ra.filt_len = d.filt_len;
    ra.oversample = d.oversample;
    ra.sinc = sinc.p;
    ra.sinc_len = d.resample ? (int)d.sinc.size() : 0;
    ra.tab4 = tab4.p;
    ra.lds_floats = ola_lds_floats;
    ra.tab_bytes = res_tab_bytes(d);
    ra.fast = fast_chain() ? 1 : 0; // (the modes with a free-form fused kernel: none of them can put NaN into the stream)
    return ra;
}

void Core::launch_chunk(const InAddr &ia, int64_t t0, int Tn, const int32_t *d_pinc, const OlaTile *d_tiles,
                        int ntiles, const int64_t *d_P, const float *d_wacc, const float *d_whisper,
                        const InAddr *carrier, float *out, int64_t out_stride_row, int64_t k_base,
                        hipStream_t st, hipEvent_t *ev, int part, hipStream_t st_chain, hipEvent_t ev_match,
                        hipEvent_t ev_chain, bool single_launch, const ChainLaunch *chain) const {
    // part 3 / 4: the back of a chunk in two pieces (fused path: 3 = everything up to the fused synthesis +
    // overlap-add kernel, 4 = the resampling kernel), for the three-stage order of pv_batch_run
    // part 5: only the rotation chain's hand-over to the second stream (for the order in which the chain starts behind
    // the previous chunk's fused kernel rather than right behind its own match kernel: ChainLaunch::late_chain)
    // part 6 / 7: the front of a chunk in two pieces (6 = the analysis kernel only, 7 = match kernel + the rotation
    // chain's hand-over), for the order in which the analysis runs one chunk further ahead (pv_batch_run, ahead order)
    const bool only_resample = part == 4, no_resample = part == 3, only_chain = part == 5;
    const bool only_analysis = part == 6, no_analysis = part == 7;
    const bool defer_chain = part == 1 && chain && chain->late_chain;
    if (part == 3 || part == 4) part = 2;
    if (part == 5 || part == 6 || part == 7) part = 1;
    const bool front = part != 2, back = part != 1;
    StreamArgs fused{};
    const int cm = phase_mode(d);
    auto rec = [&](int i) {
        if (ev) HIPV(hipEventRecord(ev[i], st));
    };
    // the phase stage's latency-bound kernel: on `st` (part 0), or handed to the second stream after what the
    // main stream has launched so far (part 1) and waited for before what follows (part 2)
    auto side_stream = [&](int k, auto &&launch_on) {
        if (defer_chain) return;
        if (part == 1) {
            HIPV(hipEventRecord(ev_match, st));
            HIPV(hipStreamWaitEvent(st_chain, ev_match, 0));
            if (ev) HIPV(hipEventRecord(ev[2 * k], st_chain));
            launch_on(st_chain);
            if (ev) HIPV(hipEventRecord(ev[2 * k + 1], st_chain));
            HIPV(hipEventRecord(ev_chain, st_chain));
        } else if (part == 2) {
            if (!only_resample) HIPV(hipStreamWaitEvent(st, ev_chain, 0));
        } else {
            rec(2 * k);
            launch_on(st);
            rec(2 * k + 1);
        }
    };
    // every stage's block: the Core's builder, then what belongs to this launch
    const int s0 = (int)(t0 % TR);
    AnalyzeArgs aa = analyze_args(rows);
    aa.ia = ia;
    aa.t0 = t0;
    aa.s0 = s0;
    aa.Tn = Tn;
    const bool do_analysis = front && !only_chain && !no_analysis;
    if (do_analysis) rec(2 * PV_K_ANALYZE);
    if (single_launch) fused.aa = aa;
    else if (do_analysis) launch_analyze(aa, st); HIPV(hipGetLastError());
    if (do_analysis && d.vocoder && carrier) {
        // the carrier is one more (data-independent) row: same analysis, its own planes
        AnalyzeArgs ca = aa;
        ca.ia = *carrier;
        ca.rows = 1;
        ca.find_peaks = 0;
        ca.mag = cmag.p;
        ca.phase = cphase.p;
        launch_analyze(ca, st); HIPV(hipGetLastError());
    }
    if (do_analysis) rec(2 * PV_K_ANALYZE + 1);
    if (only_analysis) return;

    if (cm == 1) {
        MatchArgs ma = match_args(rows);
        ma.t0 = t0;
        ma.s0 = s0;
        ma.Tn = Tn;
        ma.phase_inc = d_pinc;
        const bool phase_fused = fuse_phase && part == 0 && !single_launch && !ev; // (filled in below: needs qa)
        if (front && !only_chain) rec(2 * PV_K_MATCH);
        if (single_launch) fused.ma = ma;
        else if (front && !only_chain && !phase_fused) launch_match(ma, st); HIPV(hipGetLastError());
        if (front && !only_chain) rec(2 * PV_K_MATCH + 1);
        SeqArgs qa = seq_args(rows);
        qa.t0 = t0;
        qa.s0 = s0;
        qa.Tn = Tn;
        qa.phase_inc = d_pinc;
        { // this path's knobs (the slot-table paths keep the builder's 1 / 0)
            static const int prio = [] {
                const char *e = getenv("AUDIOMOD_PV_SEQ_PRIO");
                return e ? atoi(e) : -1;
            }();
            qa.high_prio = prio >= 0 ? prio : 1; // (measured without: no difference, 56.6 vs 56.4 ms per step)
            static const int narrow = [] {
                const char *e = getenv("AUDIOMOD_PV_SEQ_NARROW");
                return e ? atoi(e) : 0;
            }();
            qa.narrow = narrow;
        }
        if (single_launch) fused.qa = qa;
        else if (phase_fused) {
            if (!launch_phase(ma, qa, st)) { // (does not fit one workgroup's LDS: the two kernels after all)
                launch_match(ma, st); HIPV(hipGetLastError());
                launch_seq(qa, st);
            }
            HIPV(hipGetLastError());
        } else side_stream(PV_K_SEQ, [&](hipStream_t s) { launch_seq(qa, s); HIPV(hipGetLastError()); });
    } else if (cm == 0) {
        PropArgs pa = prop_args(rows);
        pa.t0 = t0;
        pa.s0 = s0;
        pa.Tn = Tn;
        pa.phase_inc = d_pinc;
        if (single_launch) fused.pa = pa;
        else side_stream(PV_K_PROP, [&](hipStream_t s) { launch_prop(pa, s); HIPV(hipGetLastError()); });
    }

    SynthArgs sa = synth_args(rows);
    sa.whisper = d.whisper ? d_whisper : nullptr;
    sa.t0 = t0;
    sa.s0 = s0;
    sa.Tn = Tn;
    sa.phase_inc = d_pinc;
    if (cepstral_on() && !only_resample) {
        CepstralArgs ca{};
        ca.tb = tb;
        ca.Tn = Tn;
        ca.TR = TR;
        ca.rows = rows;
        ca.s0 = s0;
        ca.env_comp = cepstral_env_comp();
        ca.inv_n = d.inv_n;
        ca.mag = mag.p;
        if (back) rec(2 * PV_K_CEPSTRAL);
        if (single_launch) fused.ca = ca;
        else if (back) launch_cepstral(ca, st); HIPV(hipGetLastError());
        if (back) rec(2 * PV_K_CEPSTRAL + 1);
    }
    if (chain && !single_launch) {
        if (!back) return;
        ChainArgs ca = chain_args(rows);
        ca.Tn = Tn;
        {
#ifdef PV_DIAG
            static const int diag = [] {
                const char *e = getenv("AUDIOMOD_PV_CHAIN_DIAG");
                return e ? atoi(e) : 0;
            }();
            ca.diag = diag;
#endif
        }
        ca.slices = chain->slices;
        ca.run_off = chain->run_off;
        ca.runs = chain->runs;
        ca.wden = chain->wden;
        ca.wden_hi = chain->wden_hi;
        // the ring images: this launch reads one half and writes the other (ChainArgs::st_acc_in); launches are
        // enqueued in slice order on one stream, so flipping at enqueue time is flipping in execution order
        ca.acc_sel = acc_half | (t0 == 0 ? 2 : 0);
        if (!only_resample) acc_half ^= 1;
#ifdef PV_DIAG
        // AUDIOMOD_PV_DEBUG_STALE_ACC=1 (diagnostic builds): recreate round 2's hazard on purpose -- one buffer for both
        // directions and a first launch that reads it -- to see what a run 0 that starts from the previous pass's final
        // accumulator image puts out (reset_state leaves the image alone under the same switch)
        if (debug_stale_acc()) ca.acc_sel = 4; // bit 2 (diagnostic builds): read AND write half 0, never fresh
#endif
        ca.out = chain->out;
        ca.out_stride_row = out_stride_row;
        ca.t0 = t0;
        ResArgs ra = res_args_uniform(rows);
        ra.ntiles = chain->res_ntiles;
        ra.tiles = chain->res_tiles;
        ra.otab = chain->res_otab;
        ra.out = out;
        ra.out_stride_row = out_stride_row;
        ra.k_base = k_base;
        if (d.resample && chain->res_stream && chain->ev_ring_free && !only_resample)
            HIPV(hipStreamWaitEvent(st, chain->ev_ring_free, 0));
        if (only_resample) {
        } else if (wave_fft()) {
            // synthesis and overlap-add in one kernel: the frames stay in LDS
            rec(2 * PV_K_SYNTH_OLA);
            launch_synth_chain(sa, ca, st); HIPV(hipGetLastError());
            rec(2 * PV_K_SYNTH_OLA + 1);
        } else {
            rec(2 * PV_K_SYNTH);
            launch_synth(sa, st); HIPV(hipGetLastError());
            rec(2 * PV_K_SYNTH + 1);
            rec(2 * PV_K_OLA_RESAMPLE);
            launch_frames_chain(ca, st); HIPV(hipGetLastError());
            if (!d.resample || no_resample) rec(2 * PV_K_OLA_RESAMPLE + 1);
        }
        if (no_resample) return;
        if (d.resample && chain->res_stream) {
            HIPV(hipEventRecord(chain->ev_fused, st));
            HIPV(hipStreamWaitEvent(chain->res_stream, chain->ev_fused, 0));
            if (ev && wave_fft()) HIPV(hipEventRecord(ev[2 * PV_K_OLA_RESAMPLE], chain->res_stream));
            launch_resample(ra, chain->res_stream); HIPV(hipGetLastError());
            if (ev) HIPV(hipEventRecord(ev[2 * PV_K_OLA_RESAMPLE + 1], chain->res_stream));
            HIPV(hipEventRecord(chain->ev_res, chain->res_stream));
        } else if (d.resample) {
            if (wave_fft() || only_resample) rec(2 * PV_K_OLA_RESAMPLE);
            launch_resample(ra, st); HIPV(hipGetLastError());
            rec(2 * PV_K_OLA_RESAMPLE + 1);
        }
        return;
    }
    if (back) rec(2 * PV_K_SYNTH);
    if (single_launch) fused.sa = sa;
    else if (back) launch_synth(sa, st); HIPV(hipGetLastError());
    if (back) rec(2 * PV_K_SYNTH + 1);

    OlaArgs oa{};
    oa.N = d.N;
    oa.rows = rows;
    oa.FR = FR;
    oa.frames = frames.p;
    oa.tiles = d_tiles;
    oa.P = d_P;
    oa.ntiles = ntiles;
    oa.resample = d.resample ? 1 : 0;
    oa.interp = d.interp ? 1 : 0;
    oa.num = d.res_num;
    oa.den = d.res_den;
    oa.filt_len = d.filt_len;
    oa.oversample = d.oversample;
    oa.sinc = sinc.p;
    oa.tab4 = tab4.p;
    oa.wacc = d_wacc;
    oa.sinc_len = d.resample ? (int)d.sinc.size() : 0;
    oa.lds_floats = ola_lds_floats;
    oa.wacc_pitch = wacc_pitch;
    oa.otab_off = otab_off;
    oa.tab_bytes = res_tab_bytes(d);
    oa.out = out;
    oa.out_stride_row = out_stride_row;
    oa.k_base = k_base;
    if (single_launch) {
        fused.oa = oa;
        fused.coremode = cm;
        fused.cepstral = cepstral_on() ? 1 : 0;
        launch_stream(fused, st); HIPV(hipGetLastError());
    } else if (back && ntiles > 0) {
        rec(2 * PV_K_OLA_RESAMPLE);
        launch_ola(oa, st); HIPV(hipGetLastError());
        rec(2 * PV_K_OLA_RESAMPLE + 1);
    }
}

static void fill_info(const Derived &d, int64_t slices, pv_info *o) {
    memset(o, 0, sizeof(*o));
    o->fftsize = d.N;
    o->hop_in = d.hop;
    o->hop_out_nominal = d.hop_out_nominal;
    o->outbuf_capacity = d.outbuf_cap;
    o->pitch_scale = d.pitch_scale;
    o->hs_ratio = d.hs_ratio;
    o->int_ratio = d.int_ratio;
    o->resample = d.resample;
    if (d.resample) {
        o->res_num = d.res_num;
        o->res_den = d.res_den;
        o->res_filt_len = d.filt_len;
        o->res_oversample = d.oversample;
        o->res_interp = d.interp;
    }
    o->slices = slices;
    o->bytes_per_slice = bytes_per_slice(d);
}

} // namespace pv

using namespace pv;

// ------------------------------------------------------------------------------------------
// batch engine
// ------------------------------------------------------------------------------------------
static constexpr size_t kEvPerChunk = 2 * PV_NUM_KERNELS;

struct pv_batch {
    Core core;
    BatchPlan plan;
    int64_t frames = 0;
    struct Chunk {
        int64_t t0;
        int Tn;
        int tile_begin, ntiles;
        int64_t k0; // fused path: first output of the chunk
        int res_begin, res_ntiles; // ... and its tiles of the resampling kernel
        int64_t cs_begin;          // ... its run lists in d_cs
        int run_begin, runs;       // ... and their offsets in d_run_off
        int warm;                  // ... and how many of the lists' entries are warm-up copies (pv_debug_batch_chain_runs)
    };
    DevBuf<ChainSlice> d_cs; // fused path: the run lists of every chunk
    DevBuf<int32_t> d_run_off;
    DevBuf<float> d_wden, d_wden_hi;
    DevBuf<ResTile> d_res_tiles;
    DevBuf<uint2> d_res_otab;
    std::vector<Chunk> chunks;
    DevBuf<int32_t> d_pinc;
    DevBuf<int64_t> d_P;
    DevBuf<OlaTile> d_tiles;
    DevBuf<float> d_wacc;
    DevBuf<float> d_whisper; // WHISPER mode: [slices][C][HP] host-drawn phases, shared by all streams
    DevBuf<float> d_carrier; // vocoder modes: the carrier signal for every sample fed (incl. the zero flush)
    hipStream_t chain_stream = nullptr; // second HIP stream for the rotation chain (phase-locked mode)
    hipEvent_t ev_match[4] = {}, ev_chain[4] = {};
    hipStream_t res_stream = nullptr;   // fused path, resampling configurations: the resampling kernel's stream
    hipEvent_t ev_fused[4] = {}, ev_res[4] = {};
    int timing = 0; // 0 = off, n = instrument every n-th chunk
    int64_t next_span = -1; // pv_batch_run_span: the launch the next span must start with (-1: only a first span may follow)
    int64_t tap_begin = 0, tap_end = 0; // pv_debug_batch_planes: the slices enqueued since the last launch 0
    std::vector<hipEvent_t> ev_pool; // kEvPerChunk per instrumented chunk
    std::vector<int> ev_chunk;       // chunk index of each used pool segment
    size_t ev_used = 0;
    double acc_ms[PV_NUM_KERNELS] = {};
    int64_t acc_n[PV_NUM_KERNELS] = {};
    ~pv_batch() {
        for (auto e : ev_pool) (void)hipEventDestroy(e);
        for (int i = 0; i < 4; ++i) {
            if (ev_match[i]) (void)hipEventDestroy(ev_match[i]);
            if (ev_chain[i]) (void)hipEventDestroy(ev_chain[i]);
            if (ev_fused[i]) (void)hipEventDestroy(ev_fused[i]);
            if (ev_res[i]) (void)hipEventDestroy(ev_res[i]);
        }
        if (res_stream) (void)hipStreamDestroy(res_stream);
        if (chain_stream) (void)hipStreamDestroy(chain_stream);
    }
};

struct pv_engine {
    Core core;
    int poisoned = 0; // status of a failure that left device state and host bookkeeping out of step (sticky)
    std::string poison_reason;
    std::unique_ptr<Planner> planner;
    std::unique_ptr<ChainBuilder> chain; // fused path: the running host plan of the overlap-add rings
    std::vector<SliceRec> recent; // slice table window; recent[0] is slice t_base
    int64_t t_base = 0;
    int64_t fed = 0, uploaded = 0;
    int tap_n = 0; // pv_debug_planes: slices of the most recent call that launched any, at most the planes' ring
    hipStream_t stream = nullptr;
    int ring = 0; // device input ring length (power of two) per channel
    DevBuf<float> d_in, d_out, d_whisper, d_carrier;
    PinBuf<float> h_whisper, h_carrier;
    std::unique_ptr<WhisperRng> rng;
    std::unique_ptr<CarrierGen> cargen;
    DevBuf<char> d_desc;
    PinBuf<float> h_in, h_out;
    PinBuf<char> h_desc;
    // Round 3: a call's kernels write their output straight into page-locked host memory (h_out is mapped into the
    // device's address space: out_dev) and the stream then writes a sequence number into h_flag, which pv_feed spins
    // on -- no device-to-host copy and no hipStreamSynchronize per call (AUDIOMOD_PV_STREAM_SYNC=1: the copy + the
    // synchronisation, as before).
    PinBuf<uint32_t> h_flag;
    float *out_dev = nullptr;     // device-side address of h_out
    uint32_t *flag_dev = nullptr; // ... of h_flag
    uint32_t flag_seq = 0;
    bool direct_out = false;
    int out_cap = 0; // per-row capacity of d_out / h_out
    std::vector<std::vector<float>> outq; // per channel FIFO
    size_t outq_head = 0;
    ~pv_engine() {
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// ------------------------------------------------------------------------------------------
// stream pool: many live streams, one launch sequence per call for all of them (audiomod_pv.h "Stream pool").
// One Core of `capacity` streams; slot i owns rows [i*C, (i+1)*C) of every per-row buffer and the accumulator
// images [i][2][C][AR].  Every slot keeps its own planner, overlap-add plan and accumulator half, so that it computes
// exactly what a pv_engine fed the same calls computes.
// ------------------------------------------------------------------------------------------
constexpr int kPoolDescRing = 4; // descriptor blocks of pv_pool_feed_device that may be in flight at once

struct pv_pool {
    Core core;
    int poisoned = 0;
    std::string poison_reason;
    int cap = 0, ring = 0;
    hipStream_t stream = nullptr;
    struct Slot {
        bool open = false;
        std::unique_ptr<Planner> planner;
        std::unique_ptr<ChainBuilder> chain;
        int64_t fed = 0, uploaded = 0, slices = 0;
        int tap_n = 0;    // pv_debug_pool_planes: slices of the slot's most recent launches, at most the planes' ring
        int acc_half = 0; // which accumulator half the slot's next launch reads
        std::vector<std::vector<float>> outq; // per channel FIFO
        size_t outq_head = 0;
        // the slot's derived constants: the pool's (core.d) in a uniform pool, its own in a mixed one (own_d, which
        // planner and chain reference); fast: the slot's engine would take the PV_ARITH_FAST kernels
        const Derived *d = nullptr;
        std::unique_ptr<Derived> own_d;
        bool fast = false;
        int tab = -1;              // mixed pool, resampling slot: its entry of the table arena
        int lds_floats = 0, tab_bytes = 0; // ... and its resampling kernel's LDS layout
        // the formant setting (pv_pool_set_formant): host state, read when a feed builds the slot's PoolSlot
        bool fx_on = false;
        float fx_semitones = 0.f;
        // the voice setting (pv_pool_set_voice): host state, read when a feed builds the slot's PoolSlot
        int voice = PV_VOICE_ROBOTIC;
        // the carrier setting (pv_pool_set_carrier).  A carrier slot's `d` is the vocoder engine's own derived constants
        // (own_d, in a uniform pool too), and planner and chain are built from them.  car_pos: the samples of the
        // slot's carrier its row of the carrier ring holds, [.., car_pos) -- written by the launch groups as far as
        // their frames reach, so it trails `uploaded` by what no slice has needed yet
        int carrier = PV_CARRIER_NONE;
        int64_t car_pos = 0;
    };
    std::vector<Slot> slots;
    // The carrier setting's device side, allocated by the first feed that has a carrier slot: the carrier ring
    // [cap][ring] (one row per slot: every channel's carrier is the same sequence), positions as in the input ring, and
    // the carrier planes [cap][TR][HP] that the group's carrier analysis writes and its synthesis reads.  ctab: the
    // period tables of the pool's sample rate (host; a feed with carrier slots copies them into its descriptor block)
    DevBuf<float> d_cring, d_cmag, d_cphase;
    CarrierTables ctab;
    // The voice setting's device side, allocated by the first feed (or restore) that has a whisper slot: the generator
    // state rows [cap + 1][kWhisperStatePitch] -- row `cap` is the constant fresh state, which a stream's first launch
    // reads instead of its own row -- and the phases of one launch group, [cap][kStreamChunk][C][HP]
    DevBuf<uint32_t> d_wstate;
    DevBuf<float> d_wphase;
    // Mixed pool (pv_pool_create_mixed): the range a slot's pitch / time ratio may take, and what the buffers were sized
    // for (checked again for every slot at open)
    bool mixed = false;
    pv_pool_range range{};
    int max_hop = 0, max_res_lds_floats = 0, max_res_tab_bytes = 0, max_sinc = 0, max_tab4 = 0;
    DevBuf<float> mix_stream; // the overlap-add stream rings when cfg itself does not resample
    // Table arena: entry i holds one resampling ratio's Speex table (max_sinc floats) and expanded interpolation rows
    // (max_tab4 float4), uploaded at the open that first needs the ratio and shared by every open slot with that ratio
    struct Tab {
        uint32_t num = 0, den = 0;
        int refs = 0;
    };
    std::vector<Tab> tabs;
    DevBuf<float4> d_tabs; // [capacity][tab_stride]
    size_t tab_stride = 0; // float4 per entry
    int last_launches = 0; // kernels launched by the last feed, device feed, save or restore
    DevBuf<float> d_in, d_stage; // device input rings [capacity * C][ring]; a call's packed new samples
    PinBuf<float> h_stage;
    const float *stage_src = nullptr; // what the ingest kernel reads: d_stage (or h_stage mapped, PV_POOL_MAPPED_INGEST)
    double last_host_us = 0, last_wait_us = 0; // the last pv_pool_feed: host work up to the wait, and the wait
    // One pinned and one device descriptor block.  pv_pool_feed owns `sync_desc` (the previous call has finished when
    // the next one writes it); pv_pool_feed_device returns with its launches in flight and takes the blocks of
    // `ring_desc` in turn: `done` is recorded behind the launches that read a block, and a call that finds its block
    // busy waits for that event -- the call kPoolDescRing calls back, a bounded wait.  `entry` is the event the call
    // records on the caller's stream for the pool's stream to wait for.
    struct DescBlock {
        DevBuf<char> d;
        PinBuf<char> h;
        hipEvent_t entry = nullptr, done = nullptr;
        bool busy = false;
    };
    DescBlock sync_desc, ring_desc[kPoolDescRing];
    int ring_next = 0;
    bool ring_ready = false;
    DevBuf<float> d_arena; // int16 wire: the kernels' float output [slot][C][cnt], converted by the egress kernel
    PinBuf<float> h_out; // output arena, mapped into the device's address space (out_dev)
    float *out_dev = nullptr;
    PinBuf<uint32_t> h_flag;
    uint32_t *flag_dev = nullptr;
    uint32_t flag_seq = 0;
    bool wait_value = false; // the device supports stream memory operations: spin on a flag instead of synchronising
    // Snapshots (pv_pool_save / pv_pool_restore): the device staging buffer the gather / scatter kernel works on, its
    // page-locked image (one copy per call between the two), and the call's segment table, page-locked and read by the
    // kernel through its mapping (seg_dev).  All three grow on demand.
    DevBuf<char> d_snap;
    PinBuf<char> h_snap;
    PinBuf<SnapSeg> h_seg;
    const SnapSeg *seg_dev = nullptr;
    ~pv_pool() {
        if (stream) {
            (void)hipStreamSynchronize(stream); // (device feeds may be in flight)
            (void)hipStreamDestroy(stream);
        }
        for (DescBlock &b : ring_desc) {
            if (b.entry) (void)hipEventDestroy(b.entry);
            if (b.done) (void)hipEventDestroy(b.done);
        }
    }
};

// ---------------------------------------------------------------- slot tables
// What the three slot-table forms -- stream pool, mixed pool, mixed batch -- build and launch alike.

// A descriptor block as the host writes it: every array 16-byte aligned, known by its offset
struct DescBlob {
    std::vector<char> bytes;
    int64_t put(const void *src, size_t n) {
        const size_t off = (bytes.size() + 15) & ~(size_t)15;
        bytes.resize(off + n);
        if (n) memcpy(bytes.data() + off, src, n);
        return (int64_t)off;
    }
    template <typename T> int64_t put(const std::vector<T> &v) { return put(v.data(), v.size() * sizeof(T)); }
};

// The PoolParams of a slot whose constants are `d`.  tab: the slot's entry of its table arena (a resampling slot's; the
// sinc table first, the expanded interpolation rows tab4_off float4s on)
static PoolParams slot_params(const Derived &d, int tab_bytes, int lds_floats, const float4 *tab, size_t tab4_off) {
    PoolParams q{};
    q.two_pi_hop = d.two_pi_hop;
    q.hop = d.hop;
    q.do_freq_comp = d.do_freq_comp ? 1 : 0;
    q.freq_comp = d.freq_comp;
    q.fixed_gain = d.fixed_gain;
    if (d.resample) {
        q.filt_len = d.filt_len;
        q.oversample = d.oversample;
        q.sinc_len = (int32_t)d.sinc.size();
        q.tab_bytes = tab_bytes;
        q.lds_floats = lds_floats;
        q.sinc = reinterpret_cast<const float *>(tab);
        q.tab4 = tab + tab4_off;
    }
    return q;
}

// ... and the image of such an entry, `stride` float4s: the rows expanded as Core::init expands them
static void slot_tab_image(const Derived &d, size_t stride, size_t tab4_off, std::vector<float4> &img) {
    img.assign(stride, make_float4(0, 0, 0, 0));
    memcpy(img.data(), d.sinc.data(), d.sinc.size() * sizeof(float));
    float4 *t4 = img.data() + tab4_off;
    for (int off = 0; off < d.oversample && d.interp; ++off)
        for (int j = 0; j < d.filt_len; ++j) {
            const float *sp = d.sinc.data() + 4 + (j + 1) * d.oversample - off - 2;
            t4[(size_t)off * (d.filt_len + 1) + j] = make_float4(sp[0], sp[1], sp[2], sp[3]);
        }
}

// Contiguous table entries of one kernel variant.  A launch group's table is sorted by variant_key; analysis and the
// phase stage serve every slot in one launch each, the fused synthesis + overlap-add is launched once per (frequency
// compensation, resampling, fast) present, the resampling once per (fast, interp) present within it.
struct VariantRun {
    int first, count;
    int dfc, res, fast, interp;
    int max_tiles, lds_floats, tab_bytes;
    int max_runs; // (mixed batch: the most runs a slot of the entry splits its slices into; a pool's slots have one)
};
// the variant: frequency compensation, resampling, fast kernels, interpolated table (sort order)
static int variant_key(const Derived &d, bool fast) {
    return ((d.do_freq_comp ? 1 : 0) << 3) | ((d.resample ? 1 : 0) << 2) | ((fast ? 1 : 0) << 1) |
           ((d.resample && d.interp) ? 1 : 0);
}
// entry k of a table sorted by key, folded into the table's runs (k = 0, 1, ... in turn)
static void variant_runs_add(std::vector<VariantRun> &vr, int k, int key, int res_ntiles, int lds_floats, int tab_bytes,
                             int runs) {
    if (k == 0 || key != ((vr.back().dfc << 3) | (vr.back().res << 2) | (vr.back().fast << 1) | vr.back().interp))
        vr.push_back(VariantRun{k, 0, key >> 3 & 1, key >> 2 & 1, key >> 1 & 1, key & 1, 0, 0, 0, 1});
    VariantRun &r = vr.back();
    ++r.count;
    r.max_tiles = std::max(r.max_tiles, res_ntiles);
    r.lds_floats = std::max(r.lds_floats, lds_floats);
    r.tab_bytes = std::max(r.tab_bytes, tab_bytes);
    r.max_runs = std::max(r.max_runs, runs);
}
// the entries from `a` on that share one launch of the fused kernel: consecutive, they differ in interp only
static size_t variant_group_end(const std::vector<VariantRun> &runs, size_t a) {
    size_t e = a + 1;
    while (e < runs.size() && runs[e].dfc == runs[a].dfc && runs[e].res == runs[a].res && runs[e].fast == runs[a].fast) ++e;
    return e;
}

// the end of a slot's overlap-add denominators as the chain kernel reads them: whole quads, four more entries, all 1;
// reciprocals for the fast kernels
static void finish_wden(std::vector<float> &wden, bool fast) {
    wden.resize(((wden.size() + 3) & ~(size_t)3) + 4, 1.f);
    if (fast)
        for (float &v : wden) v = 1.0f / v;
}

// A buffer that grows on demand: `floor` elements at first, doubled until `need` fit.  The contents are not kept.
static size_t grown_count(size_t have, size_t need, size_t floor) {
    size_t capn = have ? have : floor;
    while (capn < need) capn *= 2;
    return capn;
}
template <typename T> static int grow(PinBuf<T> &b, size_t need, size_t floor) { return b.alloc(grown_count(b.n, need, floor)); }
template <typename T> static int grow(DevBuf<T> &b, size_t need, size_t floor, hipStream_t st) {
    return b.alloc_on(grown_count(b.n, need, floor), st);
}

// What a launch group says of each launch.  who: "pool" / "mixed batch", in front of a failed launch's name;
// no_kernel: in front of the stage a launcher refuses; count: where the launches are counted, if anywhere;
// launch = false: nothing is launched, the launchers are only asked whether the configuration fits them.
struct LaunchCheck {
    const char *who, *no_kernel;
    int *count;
    bool launch;
    int refused(const char *stage) const {
        g_last_error = std::string(no_kernel) + stage + " kernel for this configuration";
        return PV_ERR_UNSUPPORTED;
    }
    int launched(const char *stage) const {
        if (!launch) return PV_OK;
        if (count) ++*count;
        const hipError_t e = hipGetLastError();
        return e == hipSuccess ? PV_OK : hip_fail(e, (std::string(who) + " " + stage + " launch").c_str(), __LINE__);
    }
    // accepted: what the stage's launcher returned
    int after(bool accepted, const char *stage) const { return accepted ? launched(stage) : refused(stage); }
};

// The carrier setting's planes for a launch group's synthesis (SynthArgs::cmag / cphase; PoolSlot::car_off indexes
// them): null where the group holds no carrier slot.
struct PoolCarrier {
    const float *cmag = nullptr, *cphase = nullptr;
};

// The fused synthesis + overlap-add and the resampling of a launch group whose table `pl` is sorted by variant (`runs`).
// Each launch takes the group's variant in place of stream 0's: whether to compensate, to resample, to take the fast
// kernel; the compensation factor and the gain themselves are per slot (PoolParams), the block's are neutral.
// synth(sa, ca, sub, first, max_runs) and res(ra, rs, first) launch on the entries from `first` on.
template <typename Synth, typename Res>
static int launch_variant_groups(const Core &c, const PoolLaunch &pl, const std::vector<VariantRun> &runs, float *stream,
                                 const float *whisper, const PoolCarrier &car, const LaunchCheck &lc, Synth synth, Res res) {
    int rc;
    for (size_t a = 0; a < runs.size();) {
        const size_t e = variant_group_end(runs, a);
        const VariantRun &ra0 = runs[a];
        const int nslots = runs[e - 1].first + runs[e - 1].count - ra0.first;
        const PoolLaunch sub{pl.slots + ra0.first, pl.desc, pl.out, nslots, pl.max_tn, pl.max_tiles};
        int max_runs = 1;
        for (size_t k = a; k < e; ++k) max_runs = std::max(max_runs, runs[k].max_runs);
        SynthArgs sa = c.synth_args(c.C);
        sa.do_freq_comp = ra0.dfc;
        sa.freq_comp = 1;
        sa.fixed_gain = 1;
        if (whisper) sa.whisper = whisper;
        if (car.cmag) sa.cmag = car.cmag, sa.cphase = car.cphase;
        ChainArgs ca = c.chain_args(c.C);
        ca.stream = stream;
        ca.resample = ra0.res;
        ca.fast = ra0.fast;
        if ((rc = lc.after(synth(sa, ca, sub, ra0.first, max_runs), "synthesis + overlap-add")) != PV_OK) return rc;
        for (size_t k = a; k < e && ra0.res; ++k) {
            const VariantRun &rv = runs[k];
            if (rv.max_tiles <= 0 && lc.launch) continue; // (no output completed: nothing to launch; a probe still asks)
            const PoolLaunch rs{pl.slots + rv.first, pl.desc, pl.out, rv.count, pl.max_tn, rv.max_tiles};
            ResArgs ra = c.res_args(c.C); // (not the uniform part: each slot brings its own filter set-up, PoolParams)
            ra.stream = stream;
            ra.interp = rv.interp;
            ra.lds_floats = rv.lds_floats; // (the largest of the entries' slots)
            ra.tab_bytes = rv.tab_bytes;
            ra.fast = rv.fast;
            if ((rc = lc.after(res(ra, rs, rv.first), "resampling")) != PV_OK) return rc;
        }
        a = e;
    }
    return PV_OK;
}

extern "C" {

const char *pv_strerror(int s) {
    switch (s) {
    case PV_OK: return "ok";
    case PV_ERR_INVALID_ARG: return "invalid argument";
    case PV_ERR_UNSUPPORTED: return "unsupported configuration";
    case PV_ERR_NO_DEVICE: return "no gfx950 device (no CPU fallback)";
    case PV_ERR_HIP: return "HIP runtime error";
    case PV_ERR_OUTPUT_OVERRUN: return "output ring overrun";
    default: return "unknown status";
    }
}

static int g_arith = [] {
    const char *e = getenv("AUDIOMOD_PV_EXACT");
    return (e && atoi(e) != 0) ? PV_ARITH_EXACT : PV_ARITH_FAST;
}();
int pv_set_arithmetic(int arith) {
    if (arith != PV_ARITH_FAST && arith != PV_ARITH_EXACT) return PV_ERR_INVALID_ARG;
    g_arith = arith;
    return PV_OK;
}
int pv_get_arithmetic(void) { return g_arith; }

// ---- diagnostics: the launchers' census (pv_kernels.hip) and the rung a configuration gets
static const char *const kCensusSetName[PV_CENSUS_SETS] = {"batch", "pool", "pmix", "mb"};
static std::string g_census_file, g_res_census_file;
static void census_append(const std::string &file, const std::string &out) {
    if (file.empty() || out.empty()) return;
    if (FILE *f = fopen(file.c_str(), "a")) { // one write per process: lines of concurrent processes stay whole
        fwrite(out.data(), 1, out.size(), f);
        fclose(f);
    }
}
static void census_append_at_exit() {
    std::string out, out_rungs;
    char line[160];
    static const int ncs[4] = {256, 512, 1024, 2048};
    for (int set = 0; set < PV_CENSUS_SETS; ++set) {
        for (int nc : ncs)
            for (int core = -1; core <= 3; ++core)
                for (int res = 0; res < 2; ++res)
                    for (int fast = 0; fast < 2; ++fast) {
                        const int64_t n = chain_census_count(PV_CENSUS_CHAIN, set, nc, core, res, fast);
                        if (n <= 0) continue;
                        snprintf(line, sizeof line, "chain set=%s nc=%d core=%d res=%d fast=%d count=%lld\n",
                                 kCensusSetName[set], nc, core, res, fast, (long long)n);
                        out += line;
                    }
        for (int fast = 0; fast < 2; ++fast)
            for (int interp = 0; interp < 2; ++interp) {
                const int64_t n = chain_census_count(PV_CENSUS_RESAMPLE, set, fast, interp, 0, 0);
                if (n <= 0) continue;
                snprintf(line, sizeof line, "resample set=%s fast=%d interp=%d count=%lld\n", kCensusSetName[set], fast,
                         interp, (long long)n);
                out += line;
            }
        static const char *const rungs[kResRungs] = {"ref4", "vec8", "vec16", "mfma", "vec2", "vec4"};
        for (int rung = 0; rung < kResRungs; ++rung)
            for (int interp = 0; interp < 2; ++interp)
                for (int big = 0; big < 2; ++big) {
                    const int64_t n = chain_census_count(PV_CENSUS_RESAMPLE_RUNG, set, rung, interp, big, 0);
                    if (n <= 0) continue;
                    snprintf(line, sizeof line, "resample_rung set=%s rung=%s interp=%d over64k=%d count=%lld\n",
                             kCensusSetName[set], rungs[rung], interp, big, (long long)n);
                    out_rungs += line;
                }
        for (int nc : ncs)
            for (int split = 0; split < 2; ++split) {
                const int64_t n = chain_census_count(PV_CENSUS_ANALYZE, set, nc, split, 0, 0);
                if (n <= 0) continue;
                snprintf(line, sizeof line, "analyze set=%s nc=%d split=%d count=%lld\n", kCensusSetName[set], nc, split,
                         (long long)n);
                out += line;
            }
        static const char *const forms[] = {"ring", "step", "fused", "stream"};
        static const int bs[4] = {1, 3, 4, 8};
        for (int form = 0; form < 4; ++form)
            for (int b : bs) {
                const int64_t n = chain_census_count(PV_CENSUS_PHASE, set, form, b, 0, 0);
                if (n <= 0) continue;
                snprintf(line, sizeof line, "phase set=%s form=%s b=%d count=%lld\n", kCensusSetName[set], forms[form], b,
                         (long long)n);
                out += line;
            }
    }
    // (the resampling rungs go to a file of their own: what reads AUDIOMOD_PV_CHAIN_CENSUS's file keeps finding the
    // four kinds it knows, line for line; both variables may name one file)
    census_append(g_census_file, out);
    census_append(g_res_census_file, out_rungs);
}
static const bool g_census_from_env = [] {
    const char *e = getenv("AUDIOMOD_PV_CHAIN_CENSUS"), *r = getenv("AUDIOMOD_PV_RESAMPLE_CENSUS");
    if (e && *e) g_census_file = e;
    if (r && *r) g_res_census_file = r;
    if (g_census_file.empty() && g_res_census_file.empty()) return false;
    chain_census_enable(true);
    atexit(census_append_at_exit);
    return true;
}();
int pv_debug_chain_census(int on) {
    chain_census_enable(on != 0);
    return PV_OK;
}
int64_t pv_debug_chain_census_count(int kind, int set, int a, int b, int c, int d) {
    return chain_census_count(kind, set, a, b, c, d);
}

const char *pv_last_error(void) { return g_last_error.empty() ? plan_reason() : g_last_error.c_str(); }

int pv_device_count(void) { return count_gfx950(); }

const char *pv_kernel_name(int k) {
    static const char *n[PV_NUM_KERNELS] = {"pv_analyze_kernel", "pv_match_kernel", "pv_seq_kernel",
                                            "pv_prop_kernel",    "pv_synth_kernel", "pv_ola_kernel",
                                            "pv_cepstral_kernel", "pv_synth_ola_kernel"};
    return (k >= 0 && k < PV_NUM_KERNELS) ? n[k] : "";
}

// ---- the formant setting (audiomod_pv.h "Formant setting"): what every form's entry point shares
// env_comp of a stream whose pitch scale is pitch_scale (Derived::pitch_scale) with the knob at formant_semitones:
// the ratio made as derive() makes the pitch scale (float quotient, double pow, stored float), then a float quotient
static float formant_env_comp_of(float pitch_scale, float formant_semitones) {
    const float ratio = formant_semitones != 0 ? (float)std::pow(2.0, formant_semitones / 12) : 1.0f;
    return pitch_scale / ratio;
}
static int formant_value_check(float formant_semitones) {
    if (!std::isfinite(formant_semitones) || std::fabs(formant_semitones) > 48.0f) {
        g_last_error = "formant setting: formant_semitones must be a finite number within +-48";
        return PV_ERR_INVALID_ARG;
    }
    return PV_OK;
}
// the setting belongs to the two plain modes
static int formant_scope_check(const pv_config &cfg) {
    if (cfg.mode == PV_MODE_NORMAL_SHIFT || cfg.mode == PV_MODE_NORMAL_STRETCH) return PV_OK;
    g_last_error = cfg.mode == PV_MODE_FORMANT_CEPSTRAL
                       ? "formant setting: mode FORMANT_CEPSTRAL already fixes it (env_comp = the pitch scale)"
                       : "formant setting: modes NORMAL_SHIFT and NORMAL_STRETCH only";
    return PV_ERR_UNSUPPORTED;
}
static int core_set_formant(Core &c, int on, float formant_semitones) {
    g_last_error.clear();
    plan_reason_clear();
    int st = formant_scope_check(c.d.cfg);
    if (st == PV_OK && on) st = formant_value_check(formant_semitones);
    if (st != PV_OK) return st;
    if (c.d.N < 128) { // (as mode FORMANT_CEPSTRAL: the lifter keeps 60 quefrencies)
        g_last_error = "formant setting: fftsize below 128 is not supported";
        return PV_ERR_UNSUPPORTED;
    }
    c.fx_on = on != 0;
    c.fx_env_comp = on ? formant_env_comp_of(c.d.pitch_scale, formant_semitones) : 1.0f;
    return PV_OK;
}

int pv_formant_env_comp(float pitch_semitones, float formant_semitones, float *env_comp) {
    g_last_error.clear();
    plan_reason_clear();
    if (!env_comp || !std::isfinite(pitch_semitones)) return PV_ERR_INVALID_ARG;
    const int st = formant_value_check(formant_semitones);
    if (st != PV_OK) return st;
    const float pitch_scale = pitch_semitones != 0 ? (float)std::pow(2.0, pitch_semitones / 12) : 1.0f; // derive()
    *env_comp = formant_env_comp_of(pitch_scale, formant_semitones);
    return PV_OK;
}

int pv_set_formant(pv_engine *e, int on, float formant_semitones) {
    if (!e) return PV_ERR_INVALID_ARG;
    return core_set_formant(e->core, on, formant_semitones);
}

int pv_batch_set_formant(pv_batch *b, int on, float formant_semitones) {
    if (!b) return PV_ERR_INVALID_ARG;
    Core &c = b->core;
    const bool was_on = c.fx_on;
    const float was_env = c.fx_env_comp;
    const int st = core_set_formant(c, on, formant_semitones);
    if (st != PV_OK || b->ev_used == 0) return st;
    // (instrumented chunks enqueued so far were recorded under the old setting: folded under it)
    const bool now_on = c.fx_on;
    const float now_env = c.fx_env_comp;
    c.fx_on = was_on, c.fx_env_comp = was_env;
    (void)pv_batch_kernel_times(b, nullptr, nullptr);
    c.fx_on = now_on, c.fx_env_comp = now_env;
    return PV_OK;
}

int pv_plan_simulate(const pv_config *cfg, const int32_t *n, int32_t ncalls, int32_t *avail, int32_t *shift,
                     int32_t *phase, int64_t max_slices, int64_t *nslices, pv_info *info) {
    g_last_error.clear();
    plan_reason_clear();
    if (!cfg || (ncalls > 0 && !n)) return PV_ERR_INVALID_ARG;
    Derived d;
    int st = derive(*cfg, d);
    if (st != PV_OK) return st;
    Planner pl(d);
    std::vector<SliceRec> sl;
    for (int i = 0; i < ncalls; ++i) {
        st = pl.feed(n[i], sl);
        if (st != PV_OK) return st;
        if (avail) avail[i] = pl.available();
        pl.retrieve(pl.available());
    }
    for (int64_t i = 0; i < (int64_t)sl.size() && i < max_slices; ++i) {
        if (shift) shift[i] = sl[(size_t)i].shift;
        if (phase) phase[i] = sl[(size_t)i].phase_inc;
    }
    if (nslices) *nslices = (int64_t)sl.size();
    if (info) fill_info(d, (int64_t)sl.size(), info);
    return PV_OK;
}

int pv_debug_chain_rung(const pv_config *cfg, int arith, pv_chain_rung *out) {
    g_last_error.clear();
    plan_reason_clear();
    if (!cfg || !out || (arith != PV_ARITH_FAST && arith != PV_ARITH_EXACT)) return PV_ERR_INVALID_ARG;
    Derived d;
    const int st = derive(*cfg, d);
    if (st != PV_OK) return st;
    const bool fast_arith = arith == PV_ARITH_FAST;
    out->nc = d.fft.nc;
    out->plain_core = synth_chain_plain_core(Core::chain_probe(d));
    out->resample = d.resample ? 1 : 0;
    out->fast = Core::fast_capable_of(d, fast_arith) ? 1 : 0; // ChainArgs::fast, which an all-modes launch ignores
    out->wave_bound = Core::chain_wave_bound(d, fast_arith);
    out->reciprocal_wden = Core::fast_capable_of(d, fast_arith) ? 1 : 0; // Core::fast_chain() on the fused path
    return PV_OK;
}

int pv_debug_resample_rung(const pv_config *cfg, int arith, int32_t rows, pv_resample_rung *out) {
    g_last_error.clear();
    plan_reason_clear();
    if (!cfg || !out || rows < 1 || (arith != PV_ARITH_FAST && arith != PV_ARITH_EXACT)) return PV_ERR_INVALID_ARG;
    Derived d;
    const int st = derive(*cfg, d);
    if (st != PV_OK) return st;
    memset(out, 0, sizeof *out);
    out->rung = -1;
    out->resample = d.resample ? 1 : 0;
    if (!d.resample) return PV_OK;
    // (the fused path's resampler: ResArgs::fast is Core::fast_chain(), as res_args_uniform sets it)
    const ResArgs ra = res_rung_probe(d, rows, Core::fast_capable_of(d, arith == PV_ARITH_FAST));
    const ResRung rr = resample_rung(ra);
    out->res_num = d.res_num;
    out->res_den = d.res_den;
    out->filt_len = d.filt_len;
    out->oversample = d.oversample;
    out->interp = ra.interp;
    out->tab_bytes = ra.tab_bytes;
    out->lds_floats = ra.lds_floats;
    out->rung = rr.rung;
    out->lds_bytes = (int64_t)rr.lds_bytes;
    out->refused = rr.fits ? 0 : 1;
    return rr.fits ? PV_OK : refuse_resample_lds(d, rr.lds_bytes, "resampling kernel");
}

int64_t pv_plan_table(const pv_config *cfg, int which, float *out, int64_t max) {
    g_last_error.clear();
    plan_reason_clear();
    if (!cfg || max < 0 || (max > 0 && !out)) return -(int64_t)PV_ERR_INVALID_ARG;
    Derived d;
    const int st = derive(*cfg, d);
    if (st != PV_OK) return -(int64_t)st;
    if (which == PV_TABLE_CARRIER) {
        CarrierGen gen((float)cfg->sample_rate, cfg->mode == PV_MODE_VOCODER_CHORD);
        for (int64_t i = 0; i < max; ++i) out[i] = gen.next();
        return max;
    }
    const std::vector<float> *t = which == PV_TABLE_WINDOW ? &d.window : which == PV_TABLE_SINC ? &d.sinc : nullptr;
    if (!t) return -(int64_t)PV_ERR_INVALID_ARG;
    const int64_t n = (int64_t)t->size() < max ? (int64_t)t->size() : max;
    if (n > 0) memcpy(out, t->data(), (size_t)n * sizeof(float));
    return (int64_t)t->size();
}

int pv_plan_whisper_phases(int64_t n, float *out) {
    if (n < 0 || (n > 0 && !out)) return PV_ERR_INVALID_ARG;
    WhisperRng rng;
    for (int64_t i = 0; i < n; ++i) out[i] = rng.next_phase();
    return PV_OK;
}

// ---------------------------------------------------------------- batch
int pv_batch_create(const pv_config *cfg, int32_t nstreams, int64_t frames, int32_t block, int32_t flush, int device,
                    pv_batch **out) {
    g_last_error.clear();
    plan_reason_clear();
    if (!cfg || !out || nstreams < 1 || frames < 1 || block < 1) return PV_ERR_INVALID_ARG;
    *out = nullptr;
    std::unique_ptr<pv_batch> b(new pv_batch());
    // slices per launch and row (pv_plan.cc: the span planner uses the same rule)
    const int Tc = batch_chunk_slices(*cfg, nstreams, g_arith == PV_ARITH_FAST);
    b->core.pipelined_planes = Core::pipeline_wanted(*cfg);
    b->core.fast_arith = g_arith == PV_ARITH_FAST;
    int st;
    {
        // the plan first: the overlap-add rings are sized from the advances it really contains
        Derived dd;
        if ((st = derive(*cfg, dd)) != PV_OK) return st;
        if ((st = plan_batch(dd, frames, block, flush != 0, b->plan)) != PV_OK) return st;
        int mx = 1;
        bool drops = false;
        for (const SliceRec &r : b->plan.slices) {
            mx = r.adv > mx ? r.adv : mx;
            drops = drops || r.adv == 0;
        }
        b->core.chain_max_adv = mx;
        b->core.chain_required = drops;
    }
    st = b->core.init(*cfg, device, nstreams, Tc);
    if (st != PV_OK) return st;
    Core &c = b->core;
    b->frames = frames;
    const auto &sl = b->plan.slices;
    const int64_t T = (int64_t)sl.size();
    if (!c.use_chain)
        for (const SliceRec &r : sl)
            if (r.adv == 0) {
                g_last_error = "more output pending than the reference's output ring holds (the reference drops "
                               "slices there); only the fused overlap-add path reproduces that";
                return PV_ERR_OUTPUT_OVERRUN;
            }
    std::vector<int32_t> pinc((size_t)T);
    std::vector<int64_t> P((size_t)T);
    for (int64_t t = 0; t < T; ++t) {
        pinc[(size_t)t] = sl[(size_t)t].phase_inc;
        P[(size_t)t] = sl[(size_t)t].P;
    }
    std::vector<OlaTile> tiles;
    std::vector<float> wacc;
    std::vector<ChainSlice> cs;
    std::vector<int32_t> run_off;
    std::vector<float> wden, wden_hi;
    std::vector<ResTile> res_tiles;
    std::vector<uint2> res_otab;
    ChainBuilder cb(c.d, c.chain_AR, c.chain_smask);
    for (int64_t t0 = 0; t0 < T; t0 += Tc) {
        pv_batch::Chunk ch;
        ch.t0 = t0;
        ch.Tn = (int)((T - t0) < Tc ? (T - t0) : Tc);
        ch.k0 = 0;
        ch.res_begin = ch.res_ntiles = 0;
        ch.cs_begin = 0;
        ch.run_begin = 0;
        ch.runs = 1;
        ch.warm = 0;
        const int64_t t1 = t0 + ch.Tn;
        int64_t ka = sl[(size_t)t0].K0;
        int64_t kb = sl[(size_t)(t1 - 1)].K0 + sl[(size_t)(t1 - 1)].cnt;
        if (ka > b->plan.out_frames) ka = b->plan.out_frames;
        if (kb > b->plan.out_frames) kb = b->plan.out_frames;
        ch.tile_begin = (int)tiles.size();
        if (c.use_chain) {
            ch.k0 = cb.begin_launch(sl[(size_t)t0]);
            for (int64_t t = t0; t < t1; ++t) cb.add(sl[(size_t)t], b->plan.out_frames, wden, wden_hi);
            // one workgroup per row leaves CUs idle below 256 rows: split the rows' slices into runs
            int runs_wanted = (256 + c.rows - 1) / c.rows;
            if (c.rows > 256) {
                // ... and a partly filled last round above them (320 rows: two rounds for 1.25 rounds of work): pick the
                // run count with the best product of round occupancy and useful share of a run (each later run
                // re-adds the frames that reach into its range).  320 rows: 4 runs, 11.8 -> 13.1 G samples/s.
                const double warm = (double)c.d.N / (double)(c.d.min_shift > 0 ? c.d.min_shift : 1) + 1.0;
                double best = 0.0;
                for (int r = 1; r <= 8; ++r) {
                    const double wgs = (double)c.rows * r / 256.0, len = (double)(t1 - t0) / r;
                    const double eff = wgs / std::ceil(wgs) * (r == 1 ? 1.0 : len / (len + warm));
                    if (eff > best + 1e-9) best = eff, runs_wanted = r;
                }
            }
            if (const char *e = getenv("AUDIOMOD_PV_CHAIN_RUNS")) runs_wanted = atoi(e);
            ch.cs_begin = (int64_t)cs.size();
            ch.run_begin = (int)run_off.size();
            ch.runs = cb.end_launch(runs_wanted > 32 ? 32 : runs_wanted, cs, run_off);
            for (size_t i = (size_t)ch.cs_begin; i < cs.size(); ++i) ch.warm += (cs[i].flags & 2) ? 1 : 0;
            if (c.d.resample && kb > ka) {
                ch.res_begin = (int)res_tiles.size();
                c.build_res_tiles(ka, kb, res_tiles, res_otab);
                ch.res_ntiles = (int)res_tiles.size() - ch.res_begin;
            }
        } else if (kb > ka) {
            st = c.build_tiles(sl, 0, t1, ka, kb, 0, tiles, wacc);
            if (st != PV_OK) return st;
        }
        ch.ntiles = (int)tiles.size() - ch.tile_begin;
        b->chunks.push_back(ch);
    }
    if ((st = b->d_pinc.upload(pinc)) != PV_OK) return st;
    if ((st = b->d_P.upload(P)) != PV_OK) return st;
    if ((st = b->d_tiles.upload(tiles)) != PV_OK) return st;
    if ((st = b->d_wacc.upload(wacc)) != PV_OK) return st;
    if (c.use_chain) {
        // (one spare entry each: a slice that finalises or emits nothing still prefetches its first entry)
        while (wden.size() & 3) wden.push_back(1.f), wden_hi.push_back(1.f);
        for (int i = 0; i < 4; ++i) wden.push_back(1.f), wden_hi.push_back(1.f);
        if (c.fast_chain()) { // the free-form kernel normalises by multiplying
            for (float &v : wden) v = 1.0f / v;
            for (float &v : wden_hi) v = 1.0f / v;
        }
        if ((st = b->d_cs.upload(cs)) != PV_OK) return st;
        if ((st = b->d_run_off.upload(run_off)) != PV_OK) return st;
        if ((st = b->d_wden.upload(wden)) != PV_OK) return st;
        if (cb.any_upper_skip) {
            if ((st = b->d_wden_hi.upload(wden_hi)) != PV_OK) return st;
        }
        if ((st = b->d_res_tiles.upload(res_tiles)) != PV_OK) return st;
        if ((st = b->d_res_otab.upload(res_otab)) != PV_OK) return st;
    }
    if (c.can_overlap_chain()) {
        // highest stream priority: the dispatcher must place the chain's few workgroups ahead of the thousands
        // of overlap-add tiles queued on the main stream, or the chain only starts when the tiles are done
        int prio_lo = 0, prio_hi = 0;
        HIPC(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
        HIPC(hipStreamCreateWithPriority(&b->chain_stream, hipStreamNonBlocking, prio_hi));
        for (int i = 0; i < 4; ++i) {
            HIPC(hipEventCreateWithFlags(&b->ev_match[i], hipEventDisableTiming));
            HIPC(hipEventCreateWithFlags(&b->ev_chain[i], hipEventDisableTiming));
        }
    }
    if (c.use_chain && c.d.resample) {
        // AUDIOMOD_PV_RES_STREAM=1: the resampling kernel on a stream of its own, beside the next chunk's analysis.
        // Measured: no gain -- both kernels slow down by more than the overlap returns (63.2 vs 60.8 ms per step) --
        // so it is off unless asked for.
        const char *e = getenv("AUDIOMOD_PV_RES_STREAM");
        if (e && atoi(e) != 0) {
            HIPC(hipStreamCreateWithFlags(&b->res_stream, hipStreamNonBlocking));
            for (int i = 0; i < 4; ++i) {
                HIPC(hipEventCreateWithFlags(&b->ev_fused[i], hipEventDisableTiming));
                HIPC(hipEventCreateWithFlags(&b->ev_res[i], hipEventDisableTiming));
            }
        }
    }
    if (c.d.vocoder) {
        CarrierGen gen((float)c.d.cfg.sample_rate, c.d.chord);
        std::vector<float> car((size_t)b->plan.in_frames);
        for (auto &v : car) v = gen.next();
        if ((st = b->d_carrier.upload(car)) != PV_OK) return st;
    }
    if (c.d.whisper) {
        // every stream behaves like a fresh reference process, so all of them draw the same rand() sequence:
        // slice-major, channel ch0, ch1, ..., bins 0..N/2 (whisperSlice runs inside processSliceForChannel)
        WhisperRng rng;
        std::vector<float> wp((size_t)T * c.C * c.HP, 0.f);
        for (int64_t t = 0; t < T; ++t)
            for (int ch = 0; ch < c.C; ++ch)
                for (int k = 0; k <= c.d.hs; ++k) wp[((size_t)t * c.C + ch) * c.HP + k] = rng.next_phase();
        if ((st = b->d_whisper.upload(wp)) != PV_OK) return st;
    }
    *out = b.release();
    return PV_OK;
}

void pv_batch_destroy(pv_batch *b) { delete b; }

int64_t pv_batch_out_frames(const pv_batch *b) { return b ? b->plan.out_frames : -1; }
int64_t pv_batch_slices(const pv_batch *b) { return b ? (int64_t)b->plan.slices.size() : -1; }
int32_t pv_batch_launches(const pv_batch *b) { return b ? (int32_t)b->chunks.size() : -1; }
int32_t pv_batch_pipelined(const pv_batch *b) { return b ? (b->chain_stream != nullptr ? 1 : 0) : -1; }

int pv_batch_get_info(const pv_batch *b, pv_info *info) {
    if (!b || !info) return PV_ERR_INVALID_ARG;
    fill_info(b->core.d, (int64_t)b->plan.slices.size(), info);
    return PV_OK;
}

int pv_batch_enable_timing(pv_batch *b, int on) {
    if (!b) return PV_ERR_INVALID_ARG;
    b->timing = on < 0 ? 0 : on;
    b->ev_chunk.clear();
    for (int k = 0; k < PV_NUM_KERNELS; ++k) {
        b->acc_ms[k] = 0;
        b->acc_n[k] = 0;
    }
    b->ev_used = 0;
    return PV_OK;
}

// Enqueues launches [first, first + count) of the batch on `st`.  ia addresses the input rows; `out` is where output
// frame k_base of row 0 goes, rows out_stride_row floats apart.  The whole job (pv_batch_run) and a span
// (pv_batch_run_span) differ only in these addresses and in the range: inside it the order is the same, the software
// pipeline fills at its first launch and drains at its last.  timed: pv_batch_enable_timing's events (whole runs only).
static int batch_enqueue(pv_batch *b, const InAddr &ia, float *d_out, int64_t out_stride_row, int64_t k_base,
                         size_t first, size_t count, hipStream_t st, bool timed) {
    Core &c = b->core;
    int rc;
    // Instrumentation: HIP events around each kernel of every `timing`-th chunk.  An event record costs a few
    // microseconds of stream time, so instrumenting every launch would slow the run it measures by ~10 %.
    InAddr car{};
    car.in = b->d_carrier.p;
    car.stride_c = 0;
    car.stride_s = 0;
    car.mask = ~0ull;
    car.len = (int64_t)b->d_carrier.n;
    // Software pipeline of the phase-locked path (two chunks in flight): the main stream runs the front of chunk i
    // (analysis, match), then the back of chunk i-1 (synthesis, overlap-add); the second stream walks chunk i's
    // rotation chain meanwhile, and has until the back of chunk i -- one more front later -- to finish.
    const bool piped = b->chain_stream != nullptr;
    // (indices first, pointers after the pool has stopped growing: a pointer into ev_pool taken before a later
    // push_back would dangle)
    std::vector<long> ev_index(b->chunks.size(), -1);
    for (size_t ci = first; timed && ci < first + count; ++ci) {
        if (!(b->timing > 0 && (int)(ci % (size_t)b->timing) == (b->timing / 2) % b->timing)) continue;
        const size_t need = b->ev_used + kEvPerChunk;
        bool ok = true;
        while (ok && b->ev_pool.size() < need) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) ok = false;
            else b->ev_pool.push_back(e);
        }
        if (!ok) break;
        ev_index[ci] = (long)b->ev_used;
        b->ev_used = need;
        b->ev_chunk.push_back((int)ci);
    }
    auto events_for = [&](size_t ci) -> hipEvent_t * {
        return ev_index[ci] >= 0 ? &b->ev_pool[(size_t)ev_index[ci]] : nullptr;
    };
    static const bool late_env = [] {
        const char *e = getenv("AUDIOMOD_PV_LATE_CHAIN");
        return e && atoi(e) != 0;
    }();
    const bool late = late_env && b->chain_stream != nullptr && c.use_chain && c.d.resample && c.wave_fft() &&
                      b->res_stream == nullptr && c.three_stage;
    auto launch = [&](size_t ci, hipEvent_t *ev, int part) {
        const auto &ch = b->chunks[ci];
        ChainLaunch cl{};
        if (c.use_chain) {
            cl.slices = b->d_cs.p + ch.cs_begin;
            cl.run_off = b->d_run_off.p + ch.run_begin;
            cl.runs = ch.runs;
            cl.wden = b->d_wden.p;
            cl.wden_hi = b->d_wden_hi.p ? b->d_wden_hi.p : b->d_wden.p;
            cl.res_tiles = b->d_res_tiles.p + ch.res_begin;
            cl.res_otab = b->d_res_otab.p + (size_t)ch.res_begin * kTileOut;
            cl.res_ntiles = ch.res_ntiles;
            cl.res_stream = b->res_stream;
            cl.ev_fused = b->ev_fused[ci & 3];
            cl.ev_res = b->ev_res[ci & 3];
            cl.ev_ring_free = ci >= first + 2 ? b->ev_res[(ci - 2) & 3] : nullptr;
            cl.late_chain = late;
            cl.out = d_out + (ch.k0 - k_base);
        }
        c.launch_chunk(ia, ch.t0, ch.Tn, b->d_pinc.p + ch.t0, b->d_tiles.p + ch.tile_begin, ch.ntiles, b->d_P.p,
                       b->d_wacc.p + (size_t)ch.tile_begin * c.wacc_pitch,
                       b->d_whisper.p ? b->d_whisper.p + (size_t)ch.t0 * c.C * c.HP : nullptr,
                       c.d.vocoder ? &car : nullptr, d_out, out_stride_row, k_base, st, ev, part, b->chain_stream,
                       b->ev_match[ci & 3], b->ev_chain[ci & 3], false, c.use_chain ? &cl : nullptr);
    };
    // (f = the range's first launch, nchunks = one past its last: the loops below are pv_batch_run's with 0 -> f)
    const size_t f = first, nchunks = first + count;
    if (piped) {
        // the chain stream must not start before the caller's stream has reached this run (state reset, inputs)
        // Fused path with a resampling kernel: three stages -- front of chunk i, resampling of chunk i-2, fused
        // kernel of chunk i-1 -- so that the rotation chain of chunk i (started behind its match kernel) runs
        // beside the resampling kernel, whose workgroups leave it room on every CU, and is done when the fused
        // kernel, which fills the CUs' LDS, starts.
        const bool three = c.use_chain && c.d.resample && c.wave_fft() && b->res_stream == nullptr && c.three_stage;
        std::vector<hipEvent_t *> evs(nchunks, nullptr);
        const bool ahead = three && c.ahead && !late;
        if (ahead) {
            for (size_t ci = f; ci < nchunks; ++ci) evs[ci] = events_for(ci);
            if (nchunks > f) launch(f, evs[f], 6); // A(f)
            for (size_t ci = f; ci < nchunks; ++ci) {
                launch(ci, evs[ci], 7);                                  // M(ci), chain(ci) handed to its stream
                if (ci > f + 1) launch(ci - 2, evs[ci - 2], 4);          // R(ci-2)   beside the chain
                if (ci + 1 < nchunks) launch(ci + 1, evs[ci + 1], 6);    // A(ci+1)   beside what is left of it
                if (ci > f) launch(ci - 1, evs[ci - 1], 3);              // F(ci-1)
            }
            if (nchunks > f + 1) launch(nchunks - 2, evs[nchunks - 2], 4);
            if (nchunks > f) launch(nchunks - 1, evs[nchunks - 1], 3), launch(nchunks - 1, evs[nchunks - 1], 4);
        } else {
        for (size_t ci = f; ci < nchunks; ++ci) {
            evs[ci] = events_for(ci);
            launch(ci, evs[ci], 1);
            if (three) {
                if (ci > f + 1) launch(ci - 2, evs[ci - 2], 4);
                if (ci > f) launch(ci - 1, evs[ci - 1], 3);
                if (late) launch(ci, evs[ci], 5); // the chain of chunk i starts behind the fused kernel of chunk i-1
            } else if (ci > f) {
                launch(ci - 1, evs[ci - 1], 2);
            }
        }
        if (three) {
            if (nchunks > f + 1) launch(nchunks - 2, evs[nchunks - 2], 4);
            if (nchunks > f) launch(nchunks - 1, evs[nchunks - 1], 3), launch(nchunks - 1, evs[nchunks - 1], 4);
        } else if (nchunks > f) {
            launch(nchunks - 1, evs[nchunks - 1], 2);
        }
        }
    } else {
        for (size_t ci = f; ci < nchunks; ++ci) launch(ci, events_for(ci), 0);
    }
    if (b->res_stream && c.use_chain) // the caller synchronises `st`: it has to cover the resampling stream too
        for (size_t ci = nchunks > f + 2 ? nchunks - 2 : f; ci < nchunks; ++ci)
            HIPC(hipStreamWaitEvent(st, b->ev_res[ci & 3], 0));
    if ((rc = c.take_launch_error()) != PV_OK) return rc;
    HIPC(hipGetLastError());
    if (count > 0) { // (host bookkeeping for pv_debug_batch_planes)
        if (first == 0) b->tap_begin = 0;
        b->tap_end = b->chunks[nchunks - 1].t0 + b->chunks[nchunks - 1].Tn;
    }
    return PV_OK;
}

int pv_batch_run(pv_batch *b, const float *d_in, float *d_out, void *hip_stream) {
    g_last_error.clear();
    plan_reason_clear();
    if (!b || !d_in || (!d_out && b->plan.out_frames > 0)) return PV_ERR_INVALID_ARG; // an empty output needs no buffer
    Core &c = b->core;
    hipStream_t st = (hipStream_t)hip_stream;
    HIPC(hipSetDevice(c.device));
    b->next_span = -1; // a whole run in between restarts the spans
    int rc = c.reset_state(st);
    if (rc != PV_OK) return rc;
    InAddr ia;
    ia.in = d_in;
    ia.stride_c = b->frames;
    ia.stride_s = b->frames * c.C;
    ia.mask = ~0ull;
    ia.len = b->frames;
    return batch_enqueue(b, ia, d_out, b->plan.out_frames, 0, 0, b->chunks.size(), st, true);
}

int64_t pv_batch_plan_spans(const pv_config *cfg, int32_t nstreams, int64_t frames, int32_t block, int32_t flush,
                            int32_t launches_per_span, pv_batch_span_info *out, int64_t max) {
    g_last_error.clear();
    plan_reason_clear();
    if (!cfg || nstreams < 1 || frames < 1 || block < 1 || launches_per_span < 1 || max < 0 || (max > 0 && !out))
        return -(int64_t)PV_ERR_INVALID_ARG;
    Derived d;
    BatchPlan bp;
    int st;
    if ((st = derive(*cfg, d)) != PV_OK) return -(int64_t)st;
    if ((st = plan_batch(d, frames, block, flush != 0, bp)) != PV_OK) return -(int64_t)st;
    const int Tc = batch_chunk_slices(*cfg, nstreams, g_arith == PV_ARITH_FAST);
    const int64_t L = batch_launches(bp, Tc);
    int64_t count = 0;
    if (L == 0) { // no slices: one empty span
        pv_batch_span_info e;
        if ((st = batch_span(d, bp, frames, Tc, 0, 0, e)) != PV_OK) return -(int64_t)st;
        if (max > 0) out[0] = e;
        return 1;
    }
    for (int64_t f = 0; f < L; f += launches_per_span, ++count) {
        const int64_t n = L - f < launches_per_span ? L - f : launches_per_span;
        pv_batch_span_info e;
        if ((st = batch_span(d, bp, frames, Tc, (int32_t)f, (int32_t)n, e)) != PV_OK) return -(int64_t)st;
        if (count < max) out[count] = e;
    }
    return count;
}

int pv_batch_span(const pv_batch *b, int32_t first_launch, int32_t launches, pv_batch_span_info *out) {
    if (!b || !out) return PV_ERR_INVALID_ARG;
    return batch_span(b->core.d, b->plan, b->frames, b->core.Tc, first_launch, launches, *out);
}

int pv_batch_run_span(pv_batch *b, int32_t first_launch, int32_t launches, const float *d_in_win, int64_t in_pitch,
                      float *d_out_win, int64_t out_pitch, void *hip_stream) {
    g_last_error.clear();
    plan_reason_clear();
    if (!b) return PV_ERR_INVALID_ARG;
    Core &c = b->core;
    // every refusal comes before anything is enqueued or changed
    pv_batch_span_info sp;
    if (batch_span(c.d, b->plan, b->frames, c.Tc, first_launch, launches, sp) != PV_OK) return PV_ERR_INVALID_ARG;
    if (first_launch != 0 && (int64_t)first_launch != b->next_span) {
        g_last_error = "pv_batch_run_span: a span must start at launch 0 or follow the previous span";
        return PV_ERR_INVALID_ARG;
    }
    const int64_t in_len = sp.in_end - sp.in_begin, out_len = sp.out_end - sp.out_begin;
    if (in_pitch < in_len || out_pitch < out_len || in_pitch < 0 || out_pitch < 0 || (in_pitch & 3) || (out_pitch & 3) ||
        (reinterpret_cast<uintptr_t>(d_in_win) & 15u) || (reinterpret_cast<uintptr_t>(d_out_win) & 15u) ||
        (!d_in_win && in_len > 0) || (!d_out_win && out_len > 0))
        return PV_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)hip_stream;
    HIPC(hipSetDevice(c.device));
    b->next_span = -1; // (until this span is enqueued whole)
    if (first_launch == 0) {
        const int rc = c.reset_state(st);
        if (rc != PV_OK) return rc;
    }
    // The kernels address a row's input by its frame number: the window's row 0 would start in_begin floats before
    // d_in_win.  in_begin and the pitch are multiples of 4, so every row of that virtual array starts on a 16-byte
    // boundary, and the loads stay inside [in_begin, in_end) of each row (pv_plan.cc batch_span).  The length stays
    // the stream's: it is what decides between a loaded frame and a flush zero, as in the whole run.
    InAddr ia;
    // (formed as an integer: the address lies before the window's allocation, and d_in_win may be NULL for an empty range)
    ia.in = reinterpret_cast<const float *>(reinterpret_cast<uintptr_t>(d_in_win) - (uintptr_t)sp.in_begin * sizeof(float));
    ia.stride_c = in_pitch;
    ia.stride_s = in_pitch * c.C;
    ia.mask = ~0ull;
    ia.len = b->frames;
    const int rc = batch_enqueue(b, ia, d_out_win, out_pitch, sp.out_begin, (size_t)first_launch, (size_t)launches, st, false);
    if (rc != PV_OK) return rc;
    b->next_span = (int64_t)first_launch + launches;
    return PV_OK;
}

int pv_batch_kernel_times(pv_batch *b, double ms[PV_NUM_KERNELS], int64_t launches[PV_NUM_KERNELS]) {
    if (!b) return PV_ERR_INVALID_ARG;
    // fold finished event pairs into the accumulators
    const Derived &d = b->core.d;
    const int cm = phase_mode(d);
    for (size_t i = 0; i + kEvPerChunk <= b->ev_used; i += kEvPerChunk) {
        for (int k = 0; k < PV_NUM_KERNELS; ++k) {
            if ((k == PV_K_MATCH || k == PV_K_SEQ) && cm != 1) continue;
            if (k == PV_K_PROP && cm != 0) continue;
            if (k == PV_K_CEPSTRAL && !b->core.cepstral_on()) continue;
            const bool fused = b->core.use_chain && b->core.wave_fft();
            if (k == PV_K_SYNTH_OLA && !fused) continue;
            if (k == PV_K_SYNTH && fused) continue;
            if (k == PV_K_OLA_RESAMPLE && fused && !d.resample) continue; // the fused kernel emits the output itself
            if (k == PV_K_OLA_RESAMPLE && !b->core.use_chain) {
                const int ci2 = b->ev_chunk[i / kEvPerChunk];
                if (b->chunks[(size_t)ci2].ntiles == 0) continue;
            }
            float t = 0;
            if (hipEventElapsedTime(&t, b->ev_pool[i + 2 * k], b->ev_pool[i + 2 * k + 1]) == hipSuccess) {
                b->acc_ms[k] += t;
                b->acc_n[k] += 1;
            }
        }
    }
    b->ev_used = 0;
    b->ev_chunk.clear();
    for (int k = 0; k < PV_NUM_KERNELS; ++k) {
        if (ms) ms[k] = b->acc_ms[k];
        if (launches) launches[k] = b->acc_n[k];
    }
    return PV_OK;
}

// ---------------------------------------------------------------- streaming
static constexpr int kStreamChunk = 16; // slices per launch group in streaming mode

static int map_out(pv_engine *e);

int pv_create(const pv_config *cfg, int device, pv_engine **out) {
    g_last_error.clear();
    plan_reason_clear();
    if (!cfg || !out) return PV_ERR_INVALID_ARG;
    *out = nullptr;
    std::unique_ptr<pv_engine> e(new pv_engine());
    e->core.chain_required = true;
    e->core.fast_arith = g_arith == PV_ARITH_FAST; // (same kernels as the batch engine: see Core::fast_capable)
    {
        const char *ef = getenv("AUDIOMOD_PV_STREAM_FUSE_PHASE"); // =0: match kernel and rotation chain as two launches
        e->core.fuse_phase = !(ef && atoi(ef) == 0);
    }
    int st = e->core.init(*cfg, device, 1, kStreamChunk);
    if (st != PV_OK) return st;
    Core &c = e->core;
    e->planner.reset(new Planner(c.d));
    if (c.use_chain) e->chain.reset(new ChainBuilder(c.d, c.chain_AR, c.chain_smask));
    HIPC(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    e->ring = next_pow2_i(3 * c.d.N + kStreamChunk * c.d.hop + 16);
    if ((st = e->d_in.alloc((size_t)c.C * e->ring)) != PV_OK) return st;
    HIPC(hipMemset(e->d_in.p, 0, e->d_in.n * sizeof(float)));
    if ((st = e->h_in.alloc((size_t)c.C * e->ring)) != PV_OK) return st;
    // most outputs one group of slices can emit
    // (largest shift increment -- the hop itself in the modes that do not stretch, else the upper clamp
    // lrint(2 * hop * ratio), phasevocoderprocess.cc:394-395 -- through the resampler where there is one)
    const bool fixed_shift = phase_mode(c.d) < 0;
    const double max_shift = fixed_shift ? (double)c.d.hop : 2.0 * c.d.hop * c.d.hs_ratio + 1;
    const double per_slice = c.d.resample ? max_shift * c.d.res_den / c.d.res_num + 2 : max_shift + 2;
    e->out_cap = (int)(kStreamChunk * per_slice) + 64;
    if ((st = e->d_out.alloc((size_t)c.C * e->out_cap)) != PV_OK) return st;
    if ((st = e->h_out.alloc((size_t)c.C * e->out_cap)) != PV_OK) return st;
    if ((st = e->h_flag.alloc(16)) != PV_OK) return st;
    e->h_flag.p[0] = 0;
    {
        const char *es = getenv("AUDIOMOD_PV_STREAM_SYNC");
        e->direct_out = !(es && atoi(es) != 0);
    }
    if ((st = map_out(e.get())) != PV_OK) return st;
    const size_t desc_bytes = 256 * 1024; // grows on demand (ensure_desc)
    if ((st = e->d_desc.alloc(desc_bytes)) != PV_OK) return st;
    if ((st = e->h_desc.alloc(desc_bytes)) != PV_OK) return st;
    if (c.d.vocoder) {
        e->cargen.reset(new CarrierGen((float)cfg->sample_rate, c.d.chord));
        if ((st = e->d_carrier.alloc((size_t)e->ring)) != PV_OK) return st;
        HIPC(hipMemset(e->d_carrier.p, 0, (size_t)e->ring * sizeof(float)));
        if ((st = e->h_carrier.alloc((size_t)e->ring)) != PV_OK) return st;
    }
    if (c.d.whisper) {
        e->rng.reset(new WhisperRng());
        if ((st = e->d_whisper.alloc((size_t)kStreamChunk * c.C * c.HP)) != PV_OK) return st;
        if ((st = e->h_whisper.alloc((size_t)kStreamChunk * c.C * c.HP)) != PV_OK) return st;
    }
    e->outq.resize(c.C);
    *out = e.release();
    return PV_OK;
}

void pv_destroy(pv_engine *e) { delete e; }

int32_t pv_available(const pv_engine *e) { return e ? e->planner->available() : -1; }

int pv_get_info(const pv_engine *e, pv_info *info) {
    if (!e || !info) return PV_ERR_INVALID_ARG;
    fill_info(e->core.d, e->planner->slices(), info);
    return PV_OK;
}

// upload input samples [e->uploaded, upto) of the current call into the device ring
static int upload_until(pv_engine *e, const float *const *in, int64_t call_base, int64_t upto) {
    Core &c = e->core;
    while (e->uploaded < upto) {
        const int64_t pos = e->uploaded;
        const int64_t roff = pos & (e->ring - 1);
        int64_t n = upto - pos;
        if (n > e->ring - roff) n = e->ring - roff;
        for (int ch = 0; ch < c.C; ++ch)
            memcpy(e->h_in.p + (size_t)ch * e->ring + roff, in[ch] + (pos - call_base), (size_t)n * sizeof(float));
        if (e->cargen) { // the carrier advances in lock-step with the input samples
            float *hc = e->h_carrier.p + roff;
            for (int64_t i = 0; i < n; ++i) hc[i] = e->cargen->next();
            HIPC(hipMemcpyAsync(e->d_carrier.p + roff, hc, (size_t)n * sizeof(float), hipMemcpyHostToDevice, e->stream));
        }
        // one strided copy for all channels (rows of n floats, pitch = ring)
        HIPC(hipMemcpy2DAsync(e->d_in.p + roff, (size_t)e->ring * sizeof(float), e->h_in.p + roff,
                              (size_t)e->ring * sizeof(float), (size_t)n * sizeof(float), (size_t)c.C,
                              hipMemcpyHostToDevice, e->stream));
        e->uploaded += n;
    }
    return PV_OK;
}

// (re)size the pinned + device descriptor staging; contents are per launch group, nothing to preserve
static int ensure_desc(pv_engine *e, size_t bytes) {
    if (bytes <= e->h_desc.n) return PV_OK;
    size_t cap = e->h_desc.n ? e->h_desc.n : 64 * 1024;
    while (cap < bytes) cap *= 2;
    HIPC(hipStreamSynchronize(e->stream)); // an earlier group's copy may still read the old buffer
    int st = e->h_desc.alloc(cap);
    if (st != PV_OK) return st;
    return e->d_desc.alloc(cap);
}
static int map_out(pv_engine *e) { // (after h_out / h_flag were allocated)
    if (!e->direct_out) return PV_OK;
    void *p = nullptr;
    HIPC(hipHostGetDevicePointer(&p, e->h_out.p, 0));
    e->out_dev = static_cast<float *>(p);
    HIPC(hipHostGetDevicePointer(&p, e->h_flag.p, 0));
    e->flag_dev = static_cast<uint32_t *>(p);
    return PV_OK;
}
static int ensure_out(pv_engine *e, int64_t cnt) {
    if (cnt <= e->out_cap) return PV_OK;
    int cap = e->out_cap;
    while (cap < cnt) cap *= 2;
    HIPC(hipStreamSynchronize(e->stream));
    int st = e->d_out.alloc((size_t)e->core.C * cap);
    if (st != PV_OK) return st;
    if ((st = e->h_out.alloc((size_t)e->core.C * cap)) != PV_OK) return st;
    e->out_cap = cap;
    return map_out(e);
}

int pv_feed(pv_engine *e, const float *const *in, int32_t n) {
    g_last_error.clear();
    plan_reason_clear();
    if (!e || n < 0 || (n > 0 && !in)) return PV_ERR_INVALID_ARG;
    Core &c = e->core;
    if (e->poisoned) {
        g_last_error = "engine unusable after an earlier failure inside pv_feed: " + e->poison_reason;
        return e->poisoned;
    }
    HIPC(hipSetDevice(c.device));
    const int64_t call_base = e->fed;
    std::vector<SliceRec> fresh;
    // Planning is transactional: a call the planner refuses leaves the engine exactly where it was -- nothing fed,
    // nothing pending -- so the caller may retrieve and try again.
    const Planner::State before = e->planner->save();
    int st = e->planner->feed(n, fresh);
    if (st == PV_OK && !c.use_chain)
        for (const SliceRec &r : fresh)
            if (r.adv == 0) {
                g_last_error = "more output pending than the reference's output ring holds (the reference drops "
                               "slices there): retrieve between calls, or use the fused overlap-add path";
                st = PV_ERR_OUTPUT_OVERRUN;
                break;
            }
    if (st != PV_OK) {
        e->planner->restore(before);
        return st;
    }
    // From here on device state and host bookkeeping move together; a failure in between (a HIP error) cannot be
    // rolled back, so it makes the engine unusable instead of leaving it inconsistent.
    auto fail = [&](int code) {
        e->poisoned = code;
        e->poison_reason = g_last_error.empty() ? pv_strerror(code) : g_last_error;
        return code;
    };
    e->fed += n;
    const int64_t t_new0 = e->t_base + (int64_t)e->recent.size();
    e->recent.insert(e->recent.end(), fresh.begin(), fresh.end());
    const int64_t t_new1 = t_new0 + (int64_t)fresh.size();

    for (int64_t ta = t_new0; ta < t_new1; ta += kStreamChunk) {
        const int64_t tb = (t_new1 - ta) < kStreamChunk ? t_new1 : ta + kStreamChunk;
        const int Tn = (int)(tb - ta);
        // input needed by slices [ta, tb): up to (tb-1)*hop + N.  The pinned staging ring must not be
        // overwritten while a previous async copy still reads it: groups are synchronised below.
        int64_t need = (tb - 1) * (int64_t)c.d.hop + c.d.N;
        if (need > e->fed) need = e->fed;
        if ((st = upload_until(e, in, call_base, need)) != PV_OK) return fail(st);

        const SliceRec &first = e->recent[(size_t)(ta - e->t_base)];
        const SliceRec &last = e->recent[(size_t)(tb - 1 - e->t_base)];
        const int64_t ka = first.K0, kb = last.K0 + last.cnt;
        if ((st = ensure_out(e, kb - ka)) != PV_OK) return fail(st);
        // descriptors of the group, one upload: [pinc Tn int32] then either the tile path's [P list int64][tiles]
        // [window sums + output tables] or the fused path's [ChainSlice Tn][denominators][output table]
        std::vector<OlaTile> tiles;
        std::vector<float> wacc, wden, wden_hi;
        std::vector<ChainSlice> cs;
        std::vector<ResTile> res_tiles;
        std::vector<uint2> res_otab;
        if (c.use_chain) {
            e->chain->begin_launch(first);
            for (int64_t t = ta; t < tb; ++t)
                e->chain->add(e->recent[(size_t)(t - e->t_base)], INT64_MAX, wden, wden_hi);
            std::vector<int32_t> ro;
            e->chain->end_launch(1, cs, ro); // a call's few slices: one run
            if (c.d.resample && kb > ka) c.build_res_tiles(ka, kb, res_tiles, res_otab);
            while (wden.size() & 3) wden.push_back(1.f), wden_hi.push_back(1.f);
            for (int i = 0; i < 4; ++i) wden.push_back(1.f), wden_hi.push_back(1.f);
            if (c.fast_chain()) { // the free-form kernel normalises by multiplying
                for (float &v : wden) v = 1.0f / v;
                for (float &v : wden_hi) v = 1.0f / v;
            }
        } else if (kb > ka) {
            st = c.build_tiles(e->recent, e->t_base, tb, ka, kb, (int32_t)e->t_base, tiles, wacc);
            if (st != PV_OK) return fail(st);
        }
        auto pad16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
        const size_t nP = c.use_chain ? 0 : (size_t)(tb - e->t_base);
        const bool hi = c.use_chain && e->chain->any_upper_skip;
        const size_t o_pinc = 0, o_ro = pad16((size_t)Tn * 4), o_a = o_ro + 16; // (o_ro: the run offsets {0, Tn})
        const size_t o_b = o_a + (c.use_chain ? pad16(cs.size() * sizeof(ChainSlice)) : pad16(nP * 8));
        const size_t o_c = o_b + (c.use_chain ? pad16(wden.size() * 4) : pad16(tiles.size() * sizeof(OlaTile)));
        const size_t o_d = o_c + (c.use_chain ? (hi ? pad16(wden_hi.size() * 4) : 0) : pad16(wacc.size() * 4));
        const size_t o_e = o_d + (c.use_chain ? pad16(res_tiles.size() * sizeof(ResTile)) : 0);
        const size_t total = o_e + (c.use_chain ? pad16(res_otab.size() * sizeof(uint2)) : 0);
        if ((st = ensure_desc(e, total)) != PV_OK) return fail(st);
        char *hd = e->h_desc.p;
        int32_t *h_pinc = reinterpret_cast<int32_t *>(hd + o_pinc);
        for (int i = 0; i < Tn; ++i) h_pinc[i] = e->recent[(size_t)(ta + i - e->t_base)].phase_inc;
        {
            int32_t *h_ro = reinterpret_cast<int32_t *>(hd + o_ro);
            h_ro[0] = 0, h_ro[1] = (int32_t)cs.size(), h_ro[2] = h_ro[3] = 0;
        }
        if (c.use_chain) {
            memcpy(hd + o_a, cs.data(), cs.size() * sizeof(ChainSlice));
            memcpy(hd + o_b, wden.data(), wden.size() * 4);
            if (hi) memcpy(hd + o_c, wden_hi.data(), wden_hi.size() * 4);
            memcpy(hd + o_d, res_tiles.data(), res_tiles.size() * sizeof(ResTile));
            memcpy(hd + o_e, res_otab.data(), res_otab.size() * sizeof(uint2));
        } else {
            int64_t *h_P = reinterpret_cast<int64_t *>(hd + o_a);
            for (size_t i = 0; i < nP; ++i) h_P[i] = e->recent[i].P;
            memcpy(hd + o_b, tiles.data(), tiles.size() * sizeof(OlaTile));
            memcpy(hd + o_c, wacc.data(), wacc.size() * sizeof(float));
        }
        if (hipMemcpyAsync(e->d_desc.p, hd, total, hipMemcpyHostToDevice, e->stream) != hipSuccess)
            return fail(hip_fail(hipGetLastError(), "descriptor upload", __LINE__));

        if (c.d.whisper) {
            for (int i = 0; i < Tn; ++i)
                for (int ch = 0; ch < c.C; ++ch)
                    for (int k = 0; k <= c.d.hs; ++k)
                        e->h_whisper.p[((size_t)i * c.C + ch) * c.HP + k] = e->rng->next_phase();
            if (hipMemcpyAsync(e->d_whisper.p, e->h_whisper.p, (size_t)Tn * c.C * c.HP * sizeof(float),
                               hipMemcpyHostToDevice, e->stream) != hipSuccess)
                return fail(hip_fail(hipGetLastError(), "whisper upload", __LINE__));
        }
        InAddr ia;
        ia.in = e->d_in.p;
        ia.stride_c = e->ring;
        ia.stride_s = (int64_t)e->ring * c.C;
        ia.mask = (uint64_t)(e->ring - 1);
        ia.len = INT64_MAX;
        InAddr car = ia;
        car.in = e->d_carrier.p;
        car.stride_c = 0;
        car.stride_s = 0;
        ChainLaunch cl{};
        if (c.use_chain) {
            cl.slices = reinterpret_cast<const ChainSlice *>(e->d_desc.p + o_a);
            cl.run_off = reinterpret_cast<const int32_t *>(e->d_desc.p + o_ro);
            cl.runs = 1;
            cl.wden = reinterpret_cast<const float *>(e->d_desc.p + o_b);
            cl.wden_hi = hi ? reinterpret_cast<const float *>(e->d_desc.p + o_c) : cl.wden;
            cl.res_tiles = reinterpret_cast<const ResTile *>(e->d_desc.p + o_d);
            cl.res_otab = reinterpret_cast<const uint2 *>(e->d_desc.p + o_e);
            cl.res_ntiles = (int)res_tiles.size();
            cl.out = e->direct_out ? e->out_dev : e->d_out.p;
        }
        c.launch_chunk(ia, ta, Tn, reinterpret_cast<const int32_t *>(e->d_desc.p + o_pinc),
                       reinterpret_cast<const OlaTile *>(e->d_desc.p + o_b), (int)tiles.size(),
                       reinterpret_cast<const int64_t *>(e->d_desc.p + o_a),
                       reinterpret_cast<const float *>(e->d_desc.p + o_c), e->d_whisper.p,
                       c.d.vocoder ? &car : nullptr, e->direct_out ? e->out_dev : e->d_out.p, e->out_cap, ka, e->stream,
                       nullptr, 0, nullptr, nullptr,
                       nullptr, c.can_single_launch(), c.use_chain ? &cl : nullptr);
        if ((st = c.take_launch_error()) != PV_OK) return fail(st);
        const int64_t cnt = kb - ka;
        hipError_t he = hipSuccess;
        const bool last_group = tb == t_new1;
        if (e->direct_out) {
            // what the call leaves unconsumed goes to the device ring behind the last group's kernels, in front of
            // the flag: one wait per call
            if (last_group && (st = upload_until(e, in, call_base, e->fed)) != PV_OK) return fail(st);
            const uint32_t seq = ++e->flag_seq;
            he = hipStreamWriteValue32(e->stream, e->flag_dev, seq, 0);
            if (he == hipSuccess) {
                // spin on the host copy of the flag; look at the stream every ~4096 polls so that a failed launch ends the
                // wait instead of hanging it
                volatile uint32_t *fl = e->h_flag.p;
                uint32_t spins = 0;
                while (__atomic_load_n(fl, __ATOMIC_ACQUIRE) != seq) {
                    if ((++spins & 0xfffu) == 0) {
                        const hipError_t q = hipStreamQuery(e->stream);
                        if (q != hipSuccess && q != hipErrorNotReady) {
                            he = q;
                            break;
                        }
                        if (q == hipSuccess && __atomic_load_n(fl, __ATOMIC_ACQUIRE) != seq && spins > (1u << 26)) {
                            he = hipErrorUnknown; // the stream is idle and the flag never arrived
                            break;
                        }
                    }
                }
            }
        } else {
            if (cnt > 0)
                he = hipMemcpy2DAsync(e->h_out.p, (size_t)e->out_cap * sizeof(float), e->d_out.p,
                                      (size_t)e->out_cap * sizeof(float), (size_t)cnt * sizeof(float), (size_t)c.C,
                                      hipMemcpyDeviceToHost, e->stream);
            if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
        }
        if (he == hipSuccess) he = hipGetLastError();
        if (he != hipSuccess) return fail(hip_fail(he, "streaming launch group", __LINE__));
        for (int ch = 0; ch < c.C && cnt > 0; ++ch) {
            const float *src = e->h_out.p + (size_t)ch * e->out_cap;
            e->outq[(size_t)ch].insert(e->outq[(size_t)ch].end(), src, src + cnt);
        }
        // drop slice records no later group can reference
        const int64_t keep_from = tb - (c.lookback + kStreamChunk + 2);
        if (keep_from > e->t_base) {
            e->recent.erase(e->recent.begin(), e->recent.begin() + (size_t)(keep_from - e->t_base));
            e->t_base = keep_from;
        }
    }
    if (t_new1 > t_new0) e->tap_n = (int)std::min<int64_t>(t_new1 - t_new0, c.TR);
    // everything fed stays needed by later slices (at most 2N unconsumed): park it in the device ring
    if (e->uploaded < e->fed || !e->direct_out) { // (direct output: the last group's flag already covered the upload)
        if ((st = upload_until(e, in, call_base, e->fed)) != PV_OK) return fail(st);
        if (hipStreamSynchronize(e->stream) != hipSuccess) return fail(hip_fail(hipGetLastError(), "stream sync", __LINE__));
    }
    return PV_OK;
}

int32_t pv_retrieve(pv_engine *e, float *const *out, int32_t n) {
    if (!e || n < 0 || (n > 0 && !out)) return -1;
    // never hand out more than the FIFO holds (the planner's count and the FIFO move together; this is the guard
    // against that invariant ever breaking, not a normal path)
    const size_t held = e->outq.empty() ? 0 : e->outq[0].size() - e->outq_head;
    if ((size_t)n > held) n = (int32_t)held;
    const int32_t got = e->planner->retrieve(n);
    for (int ch = 0; ch < e->core.C; ++ch) {
        const std::vector<float> &q = e->outq[(size_t)ch];
        memcpy(out[ch], q.data() + e->outq_head, (size_t)got * sizeof(float));
    }
    e->outq_head += (size_t)got;
    if (e->outq_head > (1u << 16)) {
        for (auto &q : e->outq) q.erase(q.begin(), q.begin() + (long)e->outq_head);
        e->outq_head = 0;
    }
    return got;
}

// ---------------------------------------------------------------- stream pool
// why a configuration is outside the pool's scope (nullptr: inside).  Each excluded mode needs side data that the
// per-row kernels share across rows: the vocoders' carrier planes, WHISPER's process-wide random stream, CONSTANT's
// channel-0 overrun flag; the cepstral mode and the sizes without a wave-per-frame transform have no per-slot kernels.
static const char *pool_scope(const pv_config &cfg, const Derived &d) {
    switch (cfg.mode) {
    case PV_MODE_NORMAL_SHIFT: case PV_MODE_GENDER_CHANGE: case PV_MODE_FORMANT_PRESERVE: case PV_MODE_NORMAL_STRETCH:
    case PV_MODE_ROBOTIC: break;
    case PV_MODE_VOCODER_ROSENBERG: case PV_MODE_VOCODER_CHORD:
        return "stream pool: the vocoder modes are not pooled (their carrier planes are shared by all rows)";
    case PV_MODE_WHISPER: return "stream pool: WHISPER is not pooled (its phases come from one process-wide random stream)";
    case PV_MODE_CONSTANT: return "stream pool: CONSTANT is not pooled (its overrun flag is per stream)";
    case PV_MODE_FORMANT_CEPSTRAL: return "stream pool: FORMANT_CEPSTRAL is not pooled";
    default: return "stream pool: unknown mode";
    }
    const int nc = d.fft.nc;
    if (!(nc == 256 || nc == 512 || nc == 1024 || nc == 2048))
        return "stream pool: fftsize 512 ... 4096 only (the sizes of the fused synthesis + overlap-add kernel)";
    return nullptr;
}

static bool pool_slot_ok(const pv_pool *p, int32_t slot) {
    return p && slot >= 0 && slot < p->cap && p->slots[(size_t)slot].open;
}

static int pool_launch_group(const pv_pool *p, const PoolLaunch &pl, bool launch = true, const PoolLaunch *fx = nullptr,
                             const float *whisper = nullptr, const PoolCarrier &car = PoolCarrier());

// Core::init and pool_create allocate with DevBuf::alloc, whose zero fill is on the default stream; nothing orders that
// stream against the pool's own non-blocking one.  pv_pool_create therefore ends with a wait for the fills, so that no
// fill can land on what a slot's first launches have written.  (Buffers that grow later are filled on the pool's
// stream: DevBuf::alloc_on.)
static int pool_settle() {
    HIPC(hipStreamSynchronize(nullptr));
    return PV_OK;
}

// Waits for every device feed in flight (the events of their descriptor blocks).  An error of their launches that shows
// only now is reported here, to the call that drains: it poisons the pool.
static int pool_drain(pv_pool *p) {
    for (pv_pool::DescBlock &b : p->ring_desc) {
        if (!b.busy) continue;
        b.busy = false;
        const hipError_t e = hipEventSynchronize(b.done);
        if (e != hipSuccess) {
            p->poisoned = hip_fail(e, "stream pool device feed", __LINE__);
            p->poison_reason = g_last_error;
            return p->poisoned;
        }
    }
    return PV_OK;
}

// the chain kernel's largest overlap-add advance for one set of derived constants (as Core::init computes it)
static int pool_max_adv(const Derived &d) {
    const bool fixed_shift = phase_mode(d) < 0;
    const double m = fixed_shift ? (double)d.hop : (d.int_ratio ? (double)d.hop * d.hs_ratio : 2.0 * d.hop * d.hs_ratio + 1);
    return (int)(m < d.N ? m + 1 : d.N);
}
// LDS layout of the resampling kernel for one set of derived constants (as Core::init and pool_launch_group lay it out)
static int pool_res_lds_floats(const Derived &d) { return res_tile_lds_floats(d); }
static bool pool_in_range(const pv_pool_range &r, float time_ratio, float semis) {
    return semis >= r.min_semitones && semis <= r.max_semitones && time_ratio >= r.min_time_ratio &&
           time_ratio <= r.max_time_ratio; // (false for a NaN)
}

// What a mixed pool's buffers must hold: the largest hop, overlap-add advance and resampler set-up any slot of the
// range can have.  The hops are not monotonic (derive: input hop N/4.5 or N/6 below hs_ratio 1, N/4 at 1, N/8/hs_ratio
// above), and resampling stops at 0 st, so the constants are taken at both ends of each parameter, at 0 st, at
// hs_ratio 1, and on both sides of those breakpoints; within a side of a breakpoint each is monotonic.  The resampler's
// table sizes grow with its input step, which is largest at the highest pitch; they get a margin (the Speex rate pair only
// approximates the ratio), and pv_pool_open_with checks every slot against all of them again.
struct PoolSizing {
    int max_hop = 0, max_adv = 0;
    bool any_resample = false;
    int res_lds_floats = 0, res_tab_bytes = 0, sinc = 0, tab4 = 0;
};
static void pool_size_range(const pv_config &cfg, const pv_pool_range &r, PoolSizing &z) {
    std::vector<float> ts = {r.min_time_ratio, r.max_time_ratio, cfg.time_ratio};
    std::vector<float> ss = {r.min_semitones, r.max_semitones, cfg.pitch_semitones};
    if (r.min_semitones <= 0 && 0 <= r.max_semitones)
        ss.insert(ss.end(), {0.f, std::nextafter(0.f, -1.f), std::nextafter(0.f, 1.f), -1e-3f, 1e-3f});
    if (r.min_time_ratio <= 1 && 1 <= r.max_time_ratio) ts.push_back(1.f);
    std::vector<std::pair<float, float>> pts;
    for (float t : ts)
        for (float s : ss) pts.emplace_back(t, s);
    for (float t : ts) // hs_ratio 1 and either side of it, along each time ratio
        if (t > 0) {
            const float s1 = (float)(-12.0 * std::log2((double)t));
            for (float s : {s1, std::nextafter(s1, -1e9f), std::nextafter(s1, 1e9f), s1 - 1e-3f, s1 + 1e-3f}) pts.emplace_back(t, s);
        }
    for (float s : ss) { // ... and along each pitch
        const float t1 = (float)std::pow(2.0, -s / 12.0);
        for (float t : {t1, std::nextafter(t1, 0.f), std::nextafter(t1, 1e9f), t1 * 0.999f, t1 * 1.001f}) pts.emplace_back(t, s);
    }
    double step_max = 0;
    for (const auto &pt : pts) {
        Derived d;
        pv_config c = cfg;
        // (points just outside the range only ever bound it from above: the constants are monotonic between breakpoints)
        c.time_ratio = pt.first, c.pitch_semitones = pt.second;
        if (derive(c, d) != PV_OK) continue;
        if (d.hop > z.max_hop) z.max_hop = d.hop;
        int adv = pool_max_adv(d);
        // below hs_ratio 1 the input hop is constant and the advance grows towards hs_ratio 1: bound it there
        if (d.hs_ratio < 1 && phase_mode(d) >= 0) {
            const int up = (int)(2.0 * d.hop + 2 < d.N ? 2.0 * d.hop + 2 : d.N);
            if (up > adv) adv = up;
        }
        if (adv > z.max_adv) z.max_adv = adv;
        if (d.resample) {
            z.any_resample = true;
            const double step = (double)d.res_num / (double)d.res_den;
            if (step > step_max) step_max = step;
            if (pool_res_lds_floats(d) > z.res_lds_floats) z.res_lds_floats = pool_res_lds_floats(d);
            if (res_tab_bytes(d) > z.res_tab_bytes) z.res_tab_bytes = res_tab_bytes(d);
        }
    }
    if (z.any_resample) {
        const double step = step_max * 1.001;
        const int fl = std::max(64, (int)std::ceil(64 * step) + 4); // Speex taps (resample.c:687), with margin
        z.sinc = 8 * fl + 8;                                        // oversample <= 8: direct den * taps, or ov * taps + 8
        z.tab4 = 8 * (fl + 1);
        z.res_tab_bytes = std::max(z.res_tab_bytes, 16 * z.tab4);
        z.res_lds_floats = std::max(z.res_lds_floats, (((int)(kTileOut * step) + fl + 4 + 4 + 3) & ~3) + 4);
    }
}

static int pool_create(const pv_config *cfg, const pv_pool_range *range, int32_t capacity, int device, pv_pool **out) {
    g_last_error.clear();
    plan_reason_clear();
    if (!cfg || !out) return PV_ERR_INVALID_ARG;
    *out = nullptr;
    if (capacity < 1) {
        g_last_error = "stream pool: capacity must be at least 1";
        return PV_ERR_INVALID_ARG;
    }
    PoolSizing z;
    // the configuration (and a mixed pool's range) is checked before any device call (as Core::init does)
    {
        if (range) {
            const float v[4] = {range->min_semitones, range->max_semitones, range->min_time_ratio, range->max_time_ratio};
            const char *bad = nullptr;
            for (float x : v)
                if (!std::isfinite(x)) bad = "a bound is not a finite number";
            if (!bad && (v[0] > v[1] || v[2] > v[3])) bad = "a minimum is above its maximum";
            if (!bad && !pool_in_range(*range, cfg->time_ratio, cfg->pitch_semitones))
                bad = "the configuration's own pitch / time ratio lies outside the range";
            if (bad) {
                g_last_error = std::string("stream pool range: ") + bad;
                return PV_ERR_INVALID_ARG;
            }
        }
        Derived d;
        const int st = derive(*cfg, d);
        if (st != PV_OK) return st;
        if ((int64_t)capacity * cfg->channels > 65535) {
            g_last_error = "stream pool: capacity x channels above 65535 (the kernels put the rows on grid.y)";
            return PV_ERR_INVALID_ARG;
        }
        if (const char *why = pool_scope(*cfg, d)) {
            g_last_error = why;
            return PV_ERR_UNSUPPORTED;
        }
        if (range) {
            // the range's worst case against every per-slot kernel's limits
            pool_size_range(*cfg, *range, z);
            const int PKP = ((d.hs / 3 + 2) + 7) & ~7; // (as Core::init)
            if (phase_mode(d) == 1 && !pool_phase_supported(d.hs, PKP)) {
                g_last_error = "stream pool range: the per-slot phase kernel (match + rotation chain) does not fit one workgroup";
                return PV_ERR_UNSUPPORTED;
            }
            ChainArgs probe{};
            probe.AR = d.N + 4;
            probe.waves = 1;
            if (chain_lds_bytes(probe, d.fft.nc) > 160 * 1024 - 512) {
                g_last_error = "stream pool range: the per-slot synthesis + overlap-add kernel does not fit the LDS";
                return PV_ERR_UNSUPPORTED;
            }
            const int NR = g_arith == PV_ARITH_FAST ? 8 : 4; // rows per workgroup of the resampling kernels
            if (z.any_resample && (size_t)z.res_tab_bytes + sizeof(float) * (size_t)z.res_lds_floats * NR > 160 * 1024 - 512) {
                g_last_error = "stream pool range: the per-slot resampling kernel's filter table and tile do not fit the "
                               "LDS at the range's highest pitch";
                return PV_ERR_UNSUPPORTED;
            }
            if (z.max_hop < 1 || z.max_adv < 1) {
                g_last_error = "stream pool range: no value of the range is a valid configuration";
                return PV_ERR_INVALID_ARG;
            }
        }
    }
    std::unique_ptr<pv_pool> p(new pv_pool());
    Core &c = p->core;
    c.chain_required = true;
    c.fast_arith = g_arith == PV_ARITH_FAST;
    if (range) c.chain_max_adv = z.max_adv; // (sizes the stream ring for every slot)
    int st = c.init(*cfg, device, capacity, kStreamChunk);
    if (st != PV_OK) return st;
    if (!c.use_chain || !c.wave_fft()) {
        g_last_error = "stream pool: needs the fused synthesis + overlap-add path (AUDIOMOD_PV_FUSED=0 turns it off)";
        return PV_ERR_UNSUPPORTED;
    }
    if (phase_mode(c.d) == 1 && !pool_phase_supported(c.d.hs, c.PKP)) {
        g_last_error = "stream pool: the phase-locked kernel of this configuration does not fit one workgroup";
        return PV_ERR_UNSUPPORTED;
    }
    p->cap = capacity;
    {
        PoolLaunch probe{};
        if ((st = pool_launch_group(p.get(), probe, false)) != PV_OK) return st; // (launches nothing)
    }
    HIPC(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
    p->max_hop = range ? std::max(z.max_hop, c.d.hop) : c.d.hop;
    p->ring = next_pow2_i(3 * c.d.N + kStreamChunk * p->max_hop + 16); // (as pv_create)
    if ((st = p->d_in.alloc((size_t)c.rows * p->ring)) != PV_OK) return st;
    HIPC(hipMemset(p->d_in.p, 0, p->d_in.n * sizeof(float)));
    if ((st = p->h_flag.alloc(16)) != PV_OK) return st;
    p->h_flag.p[0] = 0;
    {
        int v = 0;
        p->wait_value = hipDeviceGetAttribute(&v, hipDeviceAttributeCanUseStreamWaitValue, device) == hipSuccess && v != 0;
    }
    if (p->wait_value) {
        void *fp = nullptr;
        HIPC(hipHostGetDevicePointer(&fp, p->h_flag.p, 0));
        p->flag_dev = static_cast<uint32_t *>(fp);
    }
    if (range) {
        p->mixed = true;
        p->range = *range;
        if (z.any_resample) {
            p->max_res_lds_floats = z.res_lds_floats;
            p->max_res_tab_bytes = z.res_tab_bytes;
            p->max_sinc = z.sinc;
            p->max_tab4 = z.tab4;
            p->tab_stride = (size_t)(z.sinc + 3) / 4 + (size_t)z.tab4;
            if ((st = p->d_tabs.alloc((size_t)capacity * p->tab_stride)) != PV_OK) return st;
            p->tabs.assign((size_t)capacity, pv_pool::Tab());
            if (!c.stream.p)
                if ((st = p->mix_stream.alloc((size_t)c.rows * ((size_t)c.chain_smask + 1))) != PV_OK) return st;
        }
    } else {
        p->range = pv_pool_range{cfg->pitch_semitones, cfg->pitch_semitones, cfg->time_ratio, cfg->time_ratio};
    }
    p->slots.resize((size_t)capacity);
    if ((st = pool_settle()) != PV_OK) return st;
    *out = p.release();
    return PV_OK;
}

int pv_pool_create(const pv_config *cfg, int32_t capacity, int device, pv_pool **out) {
    return pool_create(cfg, nullptr, capacity, device, out);
}

int pv_pool_create_mixed(const pv_config *cfg, const pv_pool_range *range, int32_t capacity, int device, pv_pool **out) {
    if (!range) {
        g_last_error = "stream pool: no range";
        if (out) *out = nullptr;
        return PV_ERR_INVALID_ARG;
    }
    return pool_create(cfg, range, capacity, device, out);
}

void pv_pool_destroy(pv_pool *p) { delete p; }

int pv_pool_last_timing(const pv_pool *p, double *host_us, double *wait_us) {
    if (!p || !host_us || !wait_us) return PV_ERR_INVALID_ARG;
    *host_us = p->last_host_us;
    *wait_us = p->last_wait_us;
    return PV_OK;
}

int pv_pool_last_launches(const pv_pool *p, int32_t *launches) {
    if (!p || !launches) return PV_ERR_INVALID_ARG;
    *launches = p->last_launches;
    return PV_OK;
}

int32_t pv_pool_capacity(const pv_pool *p) { return p ? p->cap : -1; }

static void pool_release_tab(pv_pool *p, pv_pool::Slot &sl) {
    if (sl.tab >= 0) --p->tabs[(size_t)sl.tab].refs;
    sl.tab = -1;
}

// A mixed pool's slot: its own constants, checked against what the pool was sized for.  Host only; changes nothing in
// the pool.  (pv_pool_open_with and pv_pool_restore)
static int pool_slot_constants(const pv_pool *p, float time_ratio, float semis, std::unique_ptr<Derived> &own) {
    const Core &c = p->core;
    own.reset(new Derived());
    pv_config cs = c.d.cfg;
    cs.time_ratio = time_ratio;
    cs.pitch_semitones = semis;
    const int st = derive(cs, *own);
    if (st != PV_OK) {
        if (g_last_error.empty()) g_last_error = "stream pool: the engine refuses this pitch / time ratio";
        return st;
    }
    const Derived &d = *own;
    const char *big = d.hop > p->max_hop ? "input hop" : pool_max_adv(d) > c.chain_max_adv ? "overlap-add advance" : nullptr;
    if (!big && d.resample &&
        (pool_res_lds_floats(d) > p->max_res_lds_floats || res_tab_bytes(d) > p->max_res_tab_bytes ||
         (int)d.sinc.size() > p->max_sinc || (d.interp && d.oversample * (d.filt_len + 1) > p->max_tab4)))
        big = "resampler set-up";
    if (big) {
        g_last_error = std::string("stream pool: this pitch / time ratio's ") + big + " exceeds what the pool was sized for";
        return PV_ERR_UNSUPPORTED;
    }
    return PV_OK;
}

// A mixed pool's resampling slot: the entry of the table arena with its ratio's tables -- shared with an open slot of
// the same ratio, or a free entry, uploaded here.  The caller counts the reference.
static int pool_tab_acquire(pv_pool *p, const Derived &d, int *out) {
    const Core &c = p->core;
    int tab = -1;
    for (size_t i = 0; i < p->tabs.size() && tab < 0; ++i)
        if (p->tabs[i].refs > 0 && p->tabs[i].num == d.res_num && p->tabs[i].den == d.res_den) tab = (int)i;
    if (tab < 0) {
        for (size_t i = 0; i < p->tabs.size() && tab < 0; ++i)
            if (p->tabs[i].refs == 0) tab = (int)i;
        // (at most one entry per open slot: a free one exists)
        std::vector<float4> img;
        slot_tab_image(d, p->tab_stride, (size_t)(p->max_sinc + 3) / 4, img);
        HIPC(hipSetDevice(c.device));
        // (a free entry may still be read by the in-flight device feeds of the slot that released it)
        if (const int ds = pool_drain(p)) return ds;
        HIPC(hipMemcpy(p->d_tabs.p + (size_t)tab * p->tab_stride, img.data(), img.size() * sizeof(float4),
                       hipMemcpyHostToDevice));
        p->tabs[(size_t)tab].num = d.res_num;
        p->tabs[(size_t)tab].den = d.res_den;
    }
    *out = tab;
    return PV_OK;
}

// the slot's constants and what is built from them: planner and chain start from nothing (own: null = the pool's own)
static void pool_slot_set_constants(pv_pool *p, pv_pool::Slot &sl, std::unique_ptr<Derived> own, int tab) {
    const Core &c = p->core;
    sl.own_d = std::move(own);
    sl.d = sl.own_d ? sl.own_d.get() : &c.d;
    sl.fast = Core::fast_capable_of(*sl.d, c.fast_arith);
    sl.tab = tab;
    if (tab >= 0) ++p->tabs[(size_t)tab].refs;
    sl.lds_floats = sl.d->resample ? pool_res_lds_floats(*sl.d) : 0;
    sl.tab_bytes = res_tab_bytes(*sl.d);
    sl.planner.reset(new Planner(*sl.d));
    sl.chain.reset(new ChainBuilder(*sl.d, c.chain_AR, c.chain_smask));
}

// Makes slot s an open stream of the given constants with no history (own: a mixed pool's slot's, else null).
static void pool_slot_begin(pv_pool *p, int32_t s, std::unique_ptr<Derived> own, int tab) {
    Core &c = p->core;
    pv_pool::Slot &sl = p->slots[(size_t)s];
    pool_slot_set_constants(p, sl, std::move(own), tab);
    sl.fed = sl.uploaded = sl.slices = 0;
    sl.tap_n = 0;
    sl.acc_half = 0;
    sl.fx_on = false, sl.fx_semitones = 0.f;
    sl.voice = PV_VOICE_ROBOTIC;
    sl.carrier = PV_CARRIER_NONE, sl.car_pos = 0;
    sl.outq.assign((size_t)c.C, std::vector<float>());
    sl.outq_head = 0;
    sl.open = true;
}

// ---- snapshots (audiomod_pv.h "Stream pool snapshots"; the blob's format: pv_snapshot.h)
// The pool's side of a blob header: what every slot of this pool shares -- configuration, arithmetic setting and the
// geometry of the per-row buffers, from the pool's own values.
static void pool_snap_geometry(const pv_pool *p, snap::Header &h) {
    const Core &c = p->core;
    h.sample_rate = c.d.cfg.sample_rate;
    h.channels = c.C;
    h.mode = c.d.cfg.mode;
    h.coremode = c.d.cfg.coremode;
    h.fftsize = c.d.cfg.fftsize;
    h.hopsize = c.d.cfg.hopsize;
    h.arith = c.fast_arith ? PV_ARITH_FAST : PV_ARITH_EXACT;
    h.phase_stage = phase_mode(c.d);
    h.N = c.d.N;
    h.hs = c.d.hs;
    h.ring = p->ring;
    h.TR = c.TR;
    h.HP = c.HP;
    h.PKP = c.PKP;
    h.AR = c.chain_AR;
    h.stream_len = (c.stream.p || p->mix_stream.p) ? c.chain_smask + 1 : 0;
}
// the pool's buffer behind a blob's directory entry, and its size in bytes; slot s owns bytes
// [s * seg_bytes, (s + 1) * seg_bytes) of it (rows [s*C, (s+1)*C) of a [rows][...] buffer, image s of [slot][2][C][AR])
static char *pool_snap_buffer(const pv_pool *p, int buf, size_t *bytes) {
    const Core &c = p->core;
#define PV_SNAP_BUF(b) return *bytes = (b).n * sizeof(*(b).p), reinterpret_cast<char *>((b).p)
    switch (buf) {
    case snap::kBufIn: PV_SNAP_BUF(p->d_in);
    case snap::kBufMag: PV_SNAP_BUF(c.mag);
    case snap::kBufPhase: PV_SNAP_BUF(c.phase);
    case snap::kBufOutphase: PV_SNAP_BUF(c.outphase);
    case snap::kBufPeaks: PV_SNAP_BUF(c.peaks);
    case snap::kBufNpk: PV_SNAP_BUF(c.npk);
    case snap::kBufRecs: PV_SNAP_BUF(c.recs);
    case snap::kBufModes: PV_SNAP_BUF(c.modes);
    case snap::kBufRot: PV_SNAP_BUF(c.rot);
    case snap::kBufStPp: PV_SNAP_BUF(c.st_pp);
    case snap::kBufStPo: PV_SNAP_BUF(c.st_po);
    case snap::kBufStRot: PV_SNAP_BUF(c.st_rot);
    case snap::kBufStKind: PV_SNAP_BUF(c.st_kind);
    case snap::kBufAcc: PV_SNAP_BUF(c.st_acc);
    case snap::kBufStream:
        if (c.stream.p) PV_SNAP_BUF(c.stream);
        PV_SNAP_BUF(p->mix_stream);
    default: *bytes = 0; return nullptr;
    }
#undef PV_SNAP_BUF
}
// The directory a blob of this pool has must be the pool's buffers exactly: every entry's buffer exists and holds
// `cap` slots of the entry's size.  (A disagreement would be a bug in seg_bytes; checked before any launch, because
// the kernel takes its bounds from these sizes.)
static int pool_snap_check_buffers(const pv_pool *p, const snap::Header &h) {
    for (int b = 0; b < snap::kBufCount; ++b) {
        if (b == snap::kBufWhisper) continue; // (d_wstate: cap + 1 rows of the entry's size, made on demand)
        size_t have = 0;
        const char *base = pool_snap_buffer(p, b, &have);
        const int64_t per = snap::seg_bytes(h, b);
        if ((per != 0) != (base != nullptr) || (base && (size_t)per * (size_t)p->cap != have) || (per & 3)) {
            g_last_error = "stream pool: internal: snapshot directory entry " + std::to_string(b) + " does not match the pool's buffer";
            return PV_ERR_UNSUPPORTED;
        }
    }
    return PV_OK;
}

static int pool_open_at(pv_pool *p, float time_ratio, float semis, int32_t *slot) {
    g_last_error.clear();
    plan_reason_clear();
    if (!p || !slot) return PV_ERR_INVALID_ARG;
    if (p->poisoned) {
        g_last_error = "pool unusable after an earlier failure: " + p->poison_reason;
        return p->poisoned;
    }
    if (!pool_in_range(p->range, time_ratio, semis)) {
        g_last_error = p->mixed ? "stream pool: pitch / time ratio outside the pool's range"
                                : "stream pool: a pool from pv_pool_create takes only its configuration's pitch / time ratio";
        return PV_ERR_INVALID_ARG;
    }
    int32_t s = 0;
    while (s < p->cap && p->slots[(size_t)s].open) ++s;
    if (s == p->cap) {
        g_last_error = "stream pool: all " + std::to_string(p->cap) + " slots are open";
        return PV_ERR_INVALID_ARG;
    }
    Core &c = p->core;
    // a mixed pool's slot: its own constants, checked against what the pool was sized for (nothing changes on refusal)
    std::unique_ptr<Derived> own;
    int tab = -1;
    if (p->mixed) {
        int st = pool_slot_constants(p, time_ratio, semis, own);
        if (st != PV_OK) return st;
        if (own->resample && (st = pool_tab_acquire(p, *own, &tab)) != PV_OK) return st;
    }
    HIPC(hipSetDevice(c.device));
    // A fresh stream: the slot's rows of EVERY buffer the kernels carry between calls are zeroed (stream-ordered before
    // its first launch).  A stream's continuation reads only what pv_create and Core::reset_state zero -- the input
    // ring, st_pp, st_po, st_kind, the accumulator images -- and what the stream itself has written; the other rows are
    // cleared so that what a slot holds is a function of its own stream's history alone, whoever used the slot before
    // (a snapshot copies whole rows: pv_pool_save).
    int st = PV_OK;
    for (int b = 0; b < snap::kBufCount && st == PV_OK; ++b) {
        size_t have = 0;
        char *base = pool_snap_buffer(p, b, &have);
        const size_t per = base ? have / (size_t)p->cap : 0;
        if (!per) continue;
        const hipError_t e = hipMemsetAsync(base + (size_t)s * per, 0, per, p->stream);
        if (e != hipSuccess) st = hip_fail(e, "hipMemsetAsync", __LINE__);
    }
    if (st != PV_OK) {
        p->poisoned = st;
        p->poison_reason = g_last_error;
        return st;
    }
    pool_slot_begin(p, s, std::move(own), tab);
    *slot = s;
    return PV_OK;
}

int pv_pool_open(pv_pool *p, int32_t *slot) {
    if (!p) return PV_ERR_INVALID_ARG;
    return pool_open_at(p, p->core.d.cfg.time_ratio, p->core.d.cfg.pitch_semitones, slot);
}

int pv_pool_open_with(pv_pool *p, float time_ratio, float pitch_semitones, int32_t *slot) {
    return pool_open_at(p, time_ratio, pitch_semitones, slot);
}

int pv_pool_close(pv_pool *p, int32_t slot) {
    g_last_error.clear();
    if (!pool_slot_ok(p, slot)) {
        g_last_error = "stream pool: slot is not open";
        return PV_ERR_INVALID_ARG;
    }
    pv_pool::Slot &sl = p->slots[(size_t)slot];
    sl.open = false;
    sl.planner.reset();
    sl.chain.reset();
    pool_release_tab(p, sl);
    sl.own_d.reset();
    sl.d = nullptr;
    sl.outq.clear();
    sl.outq_head = 0;
    return PV_OK;
}

int32_t pv_pool_available(const pv_pool *p, int32_t slot) {
    return pool_slot_ok(p, slot) ? p->slots[(size_t)slot].planner->available() : -1;
}

int pv_pool_get_info(const pv_pool *p, int32_t slot, pv_info *info) {
    if (!pool_slot_ok(p, slot) || !info) return PV_ERR_INVALID_ARG;
    fill_info(*p->slots[(size_t)slot].d, p->slots[(size_t)slot].planner->slices(), info);
    return PV_OK;
}

// The slot's formant setting: host state that the next feed's descriptor building reads (pool_feed), so no device call
// and no wait for feeds in flight -- their descriptor blocks were built before the change.
int pv_pool_set_formant(pv_pool *p, int32_t slot, int on, float formant_semitones) {
    g_last_error.clear();
    plan_reason_clear();
    if (!p) return PV_ERR_INVALID_ARG;
    int st = formant_scope_check(p->core.d.cfg);
    if (st != PV_OK) return st;
    if (!pool_slot_ok(p, slot)) {
        g_last_error = "stream pool: slot " + std::to_string(slot) + " is not open";
        return PV_ERR_INVALID_ARG;
    }
    if (on && (st = formant_value_check(formant_semitones)) != PV_OK) return st;
    pv_pool::Slot &sl = p->slots[(size_t)slot];
    sl.fx_on = on != 0;
    sl.fx_semitones = on ? formant_semitones : 0.f;
    return PV_OK;
}

int pv_pool_get_formant(const pv_pool *p, int32_t slot, int *on, float *formant_semitones) {
    if (!pool_slot_ok(p, slot)) return PV_ERR_INVALID_ARG;
    const pv_pool::Slot &sl = p->slots[(size_t)slot];
    if (on) *on = sl.fx_on ? 1 : 0;
    if (formant_semitones) *formant_semitones = sl.fx_semitones;
    return PV_OK;
}

// ---- the voice setting (audiomod_pv.h "Voice setting"): what the slot-table forms share
// the state of a stream that has drawn nothing: the words that follow rand()'s 310 warm-up draws (pv_whisper.h)
static const std::vector<uint32_t> &whisper_fresh_state() {
    static const std::vector<uint32_t> fresh = [] {
        std::vector<uint32_t> v((size_t)kWhisperHist);
        WhisperRng rng;
        for (uint32_t &w : v) w = rng.next_word();
        return v;
    }();
    return fresh;
}
static int voice_scope_check(const pv_config &cfg) {
    if (cfg.mode == PV_MODE_ROBOTIC) return PV_OK;
    g_last_error = "voice setting: the voice belongs to ROBOTIC objects (create the pool or mixed batch with mode ROBOTIC)";
    return PV_ERR_UNSUPPORTED;
}
static int voice_value_check(int voice) {
    if (voice == PV_VOICE_ROBOTIC || voice == PV_VOICE_WHISPER) return PV_OK;
    g_last_error = "voice setting: unknown voice " + std::to_string(voice);
    return PV_ERR_INVALID_ARG;
}
// floats of one slot's region of the phase buffer
static size_t pool_wphase_stride(const pv_pool *p) { return (size_t)kStreamChunk * p->core.C * p->core.HP; }
// the pool's generator buffers, made in stream order by the first call that needs them
static int pool_voice_buffers(pv_pool *p) {
    if (p->d_wstate.p && p->d_wphase.p) return PV_OK;
    int st;
    if ((st = p->d_wstate.alloc_on((size_t)(p->cap + 1) * kWhisperStatePitch, p->stream)) != PV_OK) return st;
    if ((st = p->d_wphase.alloc_on((size_t)p->cap * pool_wphase_stride(p), p->stream)) != PV_OK) return st;
    HIPC(hipMemcpyAsync(p->d_wstate.p + (size_t)p->cap * kWhisperStatePitch, whisper_fresh_state().data(),
                        (size_t)kWhisperHist * sizeof(uint32_t), hipMemcpyHostToDevice, p->stream));
    return PV_OK;
}

// The slot's voice: host state that the next feed's descriptor building reads, as the formant setting.  Only before the
// slot's first slice: a change in mid-stream has no reference to be held to.
int pv_pool_set_voice(pv_pool *p, int32_t slot, int voice) {
    g_last_error.clear();
    plan_reason_clear();
    if (!p) return PV_ERR_INVALID_ARG;
    int st = voice_scope_check(p->core.d.cfg);
    if (st != PV_OK) return st;
    if (!pool_slot_ok(p, slot)) {
        g_last_error = "stream pool: slot " + std::to_string(slot) + " is not open";
        return PV_ERR_INVALID_ARG;
    }
    if ((st = voice_value_check(voice)) != PV_OK) return st;
    pv_pool::Slot &sl = p->slots[(size_t)slot];
    if (sl.slices != 0) {
        g_last_error = "voice setting: slot " + std::to_string(slot) + " has processed slices (the voice is set before the first)";
        return PV_ERR_INVALID_ARG;
    }
    if (voice == PV_VOICE_WHISPER && sl.carrier != PV_CARRIER_NONE) {
        g_last_error = "voice setting: slot " + std::to_string(slot) + " has a carrier (a stream is one engine: vocoder or WHISPER)";
        return PV_ERR_INVALID_ARG;
    }
    sl.voice = voice;
    return PV_OK;
}

int pv_pool_get_voice(const pv_pool *p, int32_t slot, int *voice) {
    if (!pool_slot_ok(p, slot)) return PV_ERR_INVALID_ARG;
    if (voice) *voice = p->slots[(size_t)slot].voice;
    return PV_OK;
}

// ---- the carrier setting (audiomod_pv.h "Carrier setting")
static int carrier_value_check(int carrier) {
    if (carrier == PV_CARRIER_NONE || carrier == PV_CARRIER_ROSENBERG || carrier == PV_CARRIER_CHORD) return PV_OK;
    g_last_error = "carrier setting: unknown carrier " + std::to_string(carrier);
    return PV_ERR_INVALID_ARG;
}
// the mode of the engine a carrier slot is, and back (PV_CARRIER_NONE for every other mode)
static int carrier_mode(int carrier) {
    return carrier == PV_CARRIER_CHORD ? PV_MODE_VOCODER_CHORD : PV_MODE_VOCODER_ROSENBERG;
}
static int carrier_of_mode(int mode) {
    return mode == PV_MODE_VOCODER_ROSENBERG ? PV_CARRIER_ROSENBERG : mode == PV_MODE_VOCODER_CHORD ? PV_CARRIER_CHORD : PV_CARRIER_NONE;
}

// The constants of the vocoder engine a carrier slot at this time ratio and pitch is: derive() of the pool's
// configuration under the carrier's mode -- the engine's own, not a second statement of its rules -- checked against
// what the pool's launches run and what its per-row buffers were sized for.  Host only; changes nothing in the pool
// but its (lazily built) carrier tables.  (pv_pool_set_carrier and pv_pool_restore)
static int pool_carrier_constants(pv_pool *p, float time_ratio, float semis, int carrier, std::unique_ptr<Derived> &own) {
    const Core &c = p->core;
    if (!p->mixed && c.d.resample) {
        g_last_error = "carrier setting: a pool from pv_pool_create runs one resampling variant for all its slots and this "
                       "one resamples (pitch other than 0), which a vocoder stream never does: create the pool with "
                       "pv_pool_create_mixed";
        return PV_ERR_UNSUPPORTED;
    }
    own.reset(new Derived());
    pv_config cs = c.d.cfg;
    cs.mode = carrier_mode(carrier);
    cs.time_ratio = time_ratio;
    cs.pitch_semitones = semis;
    const int st = derive(cs, *own);
    if (st != PV_OK) {
        if (g_last_error.empty()) g_last_error = std::string("carrier setting: the vocoder engine refuses this pitch / time ratio: ") + plan_reason();
        return st;
    }
    const Derived &d = *own;
    if (p->ctab.v.empty()) carrier_tables(c.d.cfg.sample_rate, p->ctab);
    const char *big = d.hop > p->max_hop                         ? "input ring (the vocoder's input hop)"
                      : pool_max_adv(d) > c.chain_max_adv        ? "overlap-add rings (the vocoder's advance)"
                      : p->ctab.v.size() > (size_t)kCarrierMaxFloats ? "descriptor block (the carrier's period tables at this sample rate)"
                                                                     : nullptr;
    if (big) {
        g_last_error = std::string("carrier setting: the vocoder stream needs more of the pool's ") + big + " than the pool was sized for";
        return PV_ERR_UNSUPPORTED;
    }
    return PV_OK;
}
// the pool's carrier ring and planes, made in stream order by the first feed that needs them
static int pool_carrier_buffers(pv_pool *p) {
    if (p->d_cring.p && p->d_cmag.p && p->d_cphase.p) return PV_OK;
    const Core &c = p->core;
    int st;
    if ((st = p->d_cring.alloc_on((size_t)p->cap * p->ring, p->stream)) != PV_OK) return st;
    if ((st = p->d_cmag.alloc_on((size_t)p->cap * c.TR * c.HP, p->stream)) != PV_OK) return st;
    return p->d_cphase.alloc_on((size_t)p->cap * c.TR * c.HP, p->stream);
}

// The slot's carrier: host state that the next feed's descriptor building reads, as the voice.  The slot's constants,
// planner and chain become the vocoder engine's (or the robotic engine's again); what the slot was fed before its
// first slice stays fed.
int pv_pool_set_carrier(pv_pool *p, int32_t slot, int carrier) {
    g_last_error.clear();
    plan_reason_clear();
    if (!p) return PV_ERR_INVALID_ARG;
    if (p->core.d.cfg.mode != PV_MODE_ROBOTIC) {
        g_last_error = "carrier setting: the carrier belongs to ROBOTIC pools (create the pool with mode ROBOTIC)";
        return PV_ERR_UNSUPPORTED;
    }
    if (!pool_slot_ok(p, slot)) {
        g_last_error = "stream pool: slot " + std::to_string(slot) + " is not open";
        return PV_ERR_INVALID_ARG;
    }
    int st;
    if ((st = carrier_value_check(carrier)) != PV_OK) return st;
    pv_pool::Slot &sl = p->slots[(size_t)slot];
    if (sl.slices != 0) {
        g_last_error = "carrier setting: slot " + std::to_string(slot) + " has processed slices (the carrier is set before the first)";
        return PV_ERR_INVALID_ARG;
    }
    if (carrier != PV_CARRIER_NONE && sl.voice == PV_VOICE_WHISPER) {
        g_last_error = "carrier setting: slot " + std::to_string(slot) + " has the WHISPER voice (a stream is one engine: vocoder or WHISPER)";
        return PV_ERR_INVALID_ARG;
    }
    if (carrier == sl.carrier) return PV_OK;
    const float time_ratio = sl.d->cfg.time_ratio, semis = sl.d->cfg.pitch_semitones;
    std::unique_ptr<Derived> own;
    int tab = -1;
    if (carrier != PV_CARRIER_NONE) {
        if ((st = pool_carrier_constants(p, time_ratio, semis, carrier, own)) != PV_OK) return st;
    } else if (p->mixed) { // back to the robotic slot pv_pool_open_with made
        if ((st = pool_slot_constants(p, time_ratio, semis, own)) != PV_OK) return st;
        if (own->resample && (st = pool_tab_acquire(p, *own, &tab)) != PV_OK) return st;
    }
    const Planner::State fed = sl.planner->save(); // (no slice yet: the samples waiting for the first frame)
    pool_release_tab(p, sl);
    pool_slot_set_constants(p, sl, std::move(own), tab);
    sl.planner->restore(fed);
    sl.carrier = carrier;
    sl.car_pos = 0;
    return PV_OK;
}

int pv_pool_get_carrier(const pv_pool *p, int32_t slot, int *carrier) {
    if (!pool_slot_ok(p, slot)) return PV_ERR_INVALID_ARG;
    if (carrier) *carrier = p->slots[(size_t)slot].carrier;
    return PV_OK;
}

static int carrier_window_check(int32_t sample_rate, int carrier) {
    if (sample_rate < 1) {
        g_last_error = "carrier: sample rate below 1";
        return PV_ERR_INVALID_ARG;
    }
    if (carrier != PV_CARRIER_ROSENBERG && carrier != PV_CARRIER_CHORD) {
        g_last_error = "carrier: unknown carrier " + std::to_string(carrier) + " (ROSENBERG or CHORD)";
        return PV_ERR_INVALID_ARG;
    }
    return PV_OK;
}

// host only: the closed form itself
int pv_plan_carrier(int32_t sample_rate, int carrier, int64_t first, int64_t count, float *out) {
    g_last_error.clear();
    if (!out || first < 0 || count < 0) return PV_ERR_INVALID_ARG;
    const int st = carrier_window_check(sample_rate, carrier);
    if (st != PV_OK) return st;
    CarrierTables t;
    carrier_tables(sample_rate, t);
    const bool chord = carrier == PV_CARRIER_CHORD;
    const int base = chord ? 1 : 0;
    uint32_t r[3] = {0, 0, 0};
    for (int v = 0; v < (chord ? 3 : 1); ++v) r[v] = (uint32_t)(first % t.len[base + v]);
    for (int64_t i = 0; i < count; ++i) {
        out[i] = carrier_sample(t.v.data(), t.off, chord ? 1 : 0, r[0], r[1], r[2]);
        for (int v = 0; v < (chord ? 3 : 1); ++v)
            if (++r[v] == (uint32_t)t.len[base + v]) r[v] = 0;
    }
    return PV_OK;
}

// Diagnostics: the production carrier kernel alone, njobs windows in ONE launch, concatenated into out.
int pv_debug_carrier(int32_t sample_rate, int carrier, const int64_t *first, const int32_t *count, int32_t njobs, float *out,
                     int device) {
    g_last_error.clear();
    if (njobs < 0 || (njobs > 0 && (!first || !count)) || !out) return PV_ERR_INVALID_ARG;
    int st = carrier_window_check(sample_rate, carrier);
    if (st != PV_OK) return st;
    int64_t total = 0;
    int max_n = 0;
    for (int32_t i = 0; i < njobs; ++i) {
        if (first[i] < 0 || count[i] < 0) return PV_ERR_INVALID_ARG;
        total += count[i];
        max_n = std::max(max_n, (int)count[i]);
    }
    CarrierTables t;
    carrier_tables(sample_rate, t);
    if (t.v.size() > (size_t)kCarrierMaxFloats) {
        g_last_error = "carrier: the period tables of this sample rate exceed what a launch carries";
        return PV_ERR_UNSUPPORTED;
    }
    if (count_gfx950() <= 0) {
        g_last_error = "no gfx950 (MI355X) device visible: this library has no CPU fallback";
        return PV_ERR_NO_DEVICE;
    }
    if (total == 0) return PV_OK;
    HIPC(hipSetDevice(device));
    std::vector<CarrierJob> hj;
    int64_t off = 0;
    for (int32_t i = 0; i < njobs; ++i) {
        hj.push_back(carrier_job(t, carrier == PV_CARRIER_CHORD, first[i], count[i], off, 0u));
        off += count[i];
    }
    DevBuf<float> d_out, d_tab;
    DevBuf<CarrierJob> d_jobs;
    if ((st = d_out.alloc((size_t)total)) != PV_OK || (st = d_tab.upload(t.v)) != PV_OK || (st = d_jobs.upload(hj)) != PV_OK) return st;
    CarrierArgs a{};
    a.out = d_out.p;
    a.tab = d_tab.p;
    for (int k = 0; k < kCarrierTabs; ++k) a.off[k] = t.off[k], a.len[k] = t.len[k];
    a.mask = 0xffffffffu; // (linear: a window of fewer than 2^31 samples from pos 0)
    a.jobs = d_jobs.p;
    launch_carrier(a, njobs, max_n, nullptr);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "carrier generator launch", __LINE__);
    HIPC(hipDeviceSynchronize());
    HIPC(hipMemcpy(out, d_out.p, (size_t)total * sizeof(float), hipMemcpyDeviceToHost));
    return PV_OK;
}

// Diagnostics: the production generator kernel alone.  One stream from the fresh state, `ncalls` launches of counts[i]
// draws each with the state carried in device memory between them (the first reads the fresh row, as a slot's first
// launch does); the phases of all launches, concatenated, to out.
int pv_debug_whisper_phases(const int64_t *counts, int32_t ncalls, float *out, int device) {
    g_last_error.clear();
    if (ncalls < 0 || (ncalls > 0 && !counts)) return PV_ERR_INVALID_ARG;
    int64_t total = 0;
    for (int32_t i = 0; i < ncalls; ++i) {
        if (counts[i] < 0 || counts[i] > 0x7fffffff) return PV_ERR_INVALID_ARG;
        total += counts[i];
    }
    if (total > 0 && !out) return PV_ERR_INVALID_ARG;
    if (count_gfx950() <= 0) {
        g_last_error = "no gfx950 (MI355X) device visible: this library has no CPU fallback";
        return PV_ERR_NO_DEVICE;
    }
    HIPC(hipSetDevice(device));
    DevBuf<uint32_t> state; // rows: fresh, the stream's
    DevBuf<float> phases;
    DevBuf<WhisperJob> jobs;
    int st;
    if ((st = state.alloc(2 * (size_t)kWhisperStatePitch)) != PV_OK || (st = phases.alloc((size_t)total)) != PV_OK) return st;
    std::vector<WhisperJob> hj((size_t)ncalls);
    int64_t off = 0;
    bool first = true;
    for (int32_t i = 0; i < ncalls; ++i) {
        WhisperJob &wj = hj[(size_t)i];
        wj.src_off = first && counts[i] > 0 ? 0 : kWhisperStatePitch;
        wj.dst_off = kWhisperStatePitch;
        wj.out_off = off;
        wj.count = counts[i];
        wj.per = counts[i] > 0 ? (int32_t)counts[i] : 1, wj.pitch = 0; // (one row: draw i at out_off + i)
        if (counts[i] > 0) first = false;
        off += counts[i];
    }
    if ((st = jobs.upload(hj)) != PV_OK) return st;
    HIPC(hipMemcpy(state.p, whisper_fresh_state().data(), (size_t)kWhisperHist * sizeof(uint32_t), hipMemcpyHostToDevice));
    for (int32_t i = 0; i < ncalls; ++i) {
        if (counts[i] == 0) continue;
        launch_whisper(state.p, phases.p, jobs.p + i, 1, PV_CENSUS_SET_BATCH, 1024, nullptr);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "voice generator launch", __LINE__);
    }
    HIPC(hipDeviceSynchronize());
    if (total > 0) HIPC(hipMemcpy(out, phases.p, (size_t)total * sizeof(float), hipMemcpyDeviceToHost));
    return PV_OK;
}

int32_t pv_pool_retrieve(pv_pool *p, int32_t slot, float *const *out, int32_t n) {
    if (!pool_slot_ok(p, slot) || n < 0 || (n > 0 && !out)) return -1;
    pv_pool::Slot &sl = p->slots[(size_t)slot];
    const size_t held = sl.outq.empty() ? 0 : sl.outq[0].size() - sl.outq_head;
    if ((size_t)n > held) n = (int32_t)held;
    const int32_t got = sl.planner->retrieve(n);
    for (int ch = 0; ch < p->core.C && got > 0; ++ch)
        memcpy(out[ch], sl.outq[(size_t)ch].data() + sl.outq_head, (size_t)got * sizeof(float));
    sl.outq_head += (size_t)got;
    if (sl.outq_head > (1u << 16)) {
        for (auto &q : sl.outq) q.erase(q.begin(), q.begin() + (long)sl.outq_head);
        sl.outq_head = 0;
    }
    return got;
}

// the pool's ingest ring as the analysis kernel's input: slot s at s * stride_s, never past an end
static InAddr pool_ring_addr(const pv_pool *p) {
    InAddr ia{};
    ia.in = p->d_in.p;
    ia.stride_c = p->ring;
    ia.stride_s = (int64_t)p->ring * p->core.C;
    ia.mask = (uint64_t)(p->ring - 1);
    ia.len = INT64_MAX;
    return ia;
}

// the formant stage's block on the slot-table paths (rows = C; Tn, s0 and env_comp come from each slot's PoolSlot)
static CepstralArgs slot_cepstral_args(const Core &c) {
    CepstralArgs a{};
    a.tb = c.tb;
    a.TR = c.TR;
    a.rows = c.C;
    a.inv_n = c.d.inv_n;
    a.mag = c.mag.p;
    return a;
}

// What a pool's launch group runs once for every slot in it, whatever the slots' variants: analysis, the phase stage
// and the formant stage (Core's argument builders with rows = C).
// q: a mixed pool's PoolParams table, parallel to pl.slots (null: a uniform pool)
// fx: the table of the group's slots that run the formant stage (null: none does)
static int pool_launch_front(const pv_pool *p, const PoolLaunch &pl, const PoolParams *q, const LaunchCheck &lc,
                             const PoolLaunch *fx) {
    const Core &c = p->core;
    hipStream_t st = p->stream;
    const int cm = phase_mode(c.d);
    int rc;
    if (!lc.launch) return PV_OK; // (pv_pool_create's question goes to the launchers after these)
    AnalyzeArgs aa = c.analyze_args(c.C); // (its hop is stream 0's: a mixed pool's kernel takes each slot's from PoolParams)
    aa.ia = pool_ring_addr(p);
    if ((rc = lc.after(q ? launch_pmix_analyze(aa, pl, q, st) : launch_pool_analyze(aa, pl, st), "analysis")) != PV_OK) return rc;
    if (cm == 1) {
        const MatchArgs ma = c.match_args(c.C);
        const SeqArgs qa = c.seq_args(c.C);
        if ((rc = lc.after(q ? launch_pmix_phase(ma, qa, pl, q, st) : launch_pool_phase(ma, qa, pl, st), "phase")) != PV_OK) return rc;
    } else if (cm == 0) {
        const PropArgs pa = c.prop_args(c.C);
        if ((rc = lc.after(q ? launch_pmix_prop(pa, pl, q, st) : launch_pool_prop(pa, pl, st), "propagation")) != PV_OK) return rc;
    }
    if (!fx) return PV_OK;
    return lc.after(launch_slot_cepstral(slot_cepstral_args(c), *fx, q ? PV_CENSUS_SET_PMIX : PV_CENSUS_SET_POOL, st), "formant");
}

// the stages of a uniform pool's launch group
// launch = false: launch nothing, only ask the launchers whether this configuration fits them (pv_pool_create)
// whisper: the phase buffer where the group holds a whisper slot (PoolSlot::wh_off), drawn by the caller's generator
// launch; else null
// car: the carrier planes where the group holds a carrier slot (PoolSlot::car_off), written by pool_launch_carrier
static int pool_launch_group(const pv_pool *p, const PoolLaunch &pl, bool launch, const PoolLaunch *fx,
                             const float *whisper, const PoolCarrier &car) {
    const Core &c = p->core;
    hipStream_t st = p->stream;
    const LaunchCheck lc{"pool", "stream pool: no per-slot ", nullptr, launch};
    int rc;
    if ((rc = pool_launch_front(p, pl, nullptr, lc, fx)) != PV_OK) return rc;
    SynthArgs sa = c.synth_args(c.C);
    if (whisper) sa.whisper = whisper;
    if (car.cmag) sa.cmag = car.cmag, sa.cphase = car.cphase;
    const ChainArgs ca = c.chain_args(c.C);
    if ((rc = lc.after(launch_pool_synth_chain(sa, ca, pl, st, launch), "synthesis + overlap-add")) != PV_OK) return rc;
    if (!c.d.resample) return PV_OK;
    return lc.after(launch_pool_resample(c.res_args_uniform(c.C), pl, st, launch), "resampling");
}

// A mixed pool's launch group: the slots of the table are ordered by kernel variant (`runs`), each with its entry of
// the PoolParams table `q`.  Counts the kernels it launches in *nlaunch.
static int pool_mix_launch_group(const pv_pool *p, const PoolLaunch &pl, const PoolParams *q,
                                 const std::vector<VariantRun> &runs, int *nlaunch, const PoolLaunch *fx,
                                 const float *whisper, const PoolCarrier &car) {
    const Core &c = p->core;
    hipStream_t st = p->stream;
    const LaunchCheck lc{"pool", "stream pool: no per-slot ", nlaunch, true};
    if (const int rc = pool_launch_front(p, pl, q, lc, fx)) return rc;
    return launch_variant_groups(
        c, pl, runs, c.stream.p ? c.stream.p : p->mix_stream.p, whisper, car, lc,
        [&](const SynthArgs &sa, const ChainArgs &ca, const PoolLaunch &sub, int first, int) {
            return launch_pmix_synth_chain(sa, ca, sub, q + first, st);
        },
        [&](const ResArgs &ra, const PoolLaunch &rs, int first) { return launch_pmix_resample(ra, rs, q + first, st); });
}

// What the two entry points of a feed differ in (pv_pool_feed: host pointers in, the slots' host FIFOs out, the pool's
// own descriptor block, a wait; pv_pool_feed_device: the caller's device buffers, a block of the ring, events).
// Planning, descriptor building, variant grouping and launching are pool_feed's, for both.
struct PoolCall {
    const float *const *in = nullptr; // pv_pool_feed: in[i * C + c], n[i] host floats
    bool device = false;              // pv_pool_feed_device: ...
    const void *d_in = nullptr;       // [count][C][in_pitch] of `wire`
    void *d_out = nullptr;            // [count][C][out_pitch] of `wire`
    int64_t in_pitch = 0, out_pitch = 0;
    int wire = PV_WIRE_F32;
    hipStream_t user = nullptr;
    int32_t *out_frames = nullptr; // [count]: what the call delivers per slot
};

// One call of pool_feed: its arguments, and what each phase leaves for the ones after it.
struct PoolFeed {
    pv_pool *p;
    int32_t count;
    const int32_t *slots, *n;
    const PoolCall &io;
    std::chrono::steady_clock::time_point t_call;
    std::vector<std::vector<SliceRec>> fresh; // plan: the slices each entry's samples complete
    pv_pool::DescBlock *blk = nullptr;        // take_block
    // place: where the call's new samples are read and its output is written
    bool to_caller = false; // the kernels write the caller's rows themselves
    std::vector<int64_t> stage_off, out_base, out_cnt, k0, call_base;
    size_t stage_total = 0, out_total = 0;
    int groups = 0;
    const void *ingest_src = nullptr;
    float *launch_out = nullptr;
    // describe: the descriptors of every group, one block
    struct Group {
        int64_t table_off = 0, ingest_off = 0;
        int nslots = 0, ningest = 0, max_tn = 0, max_tiles = 0, max_in = 0;
        int64_t fx_off = 0; // the entries of the slots that run the formant stage, once more: that launch's table
        int fx_nslots = 0, fx_max_tn = 0;
        int64_t wj_off = 0; // the generator's jobs: one per whisper slot of the group
        int nwj = 0;
        // the carrier setting: the generator's jobs (one per carrier slot whose frames reach past what its row
        // holds), and the carrier analysis' table -- the group's carrier slots once more, row0 = the slot itself
        // (one carrier row per slot) -- with its PoolParams (mixed pool)
        int64_t cj_off = 0, car_off = 0, car_params_off = 0;
        int ncj = 0, max_cn = 0, car_nslots = 0, car_max_tn = 0;
        int64_t params_off = 0;     // mixed pool: the group's PoolParams table (parallel to the PoolSlot table)
        std::vector<VariantRun> vr; // ... and its variant runs
    };
    std::vector<Group> grp; // (+ the final ingest of what the call leaves unconsumed)
    bool any_whisper = false, any_carrier = false;
    int64_t ctab_off = 0; // the carrier's period tables (where a group has generator jobs)
    int64_t egress_off = 0; // int16 output: what the egress kernel converts, per entry
    int negress = 0, max_egress = 0;
    DescBlob blob;
    std::vector<PoolIngest> ingest; // the group being described: its ingest list and generator jobs
    std::vector<WhisperJob> wjobs;
    std::vector<CarrierJob> cjobs;
    std::vector<PoolSlot> car_table;
    std::vector<PoolParams> car_params;
    std::vector<int32_t> pinc, ro; // pool_describe_slot's scratch
    std::vector<float> wden, wden_hi;
    std::vector<ChainSlice> cs;
    std::vector<ResTile> res_tiles;
    std::vector<uint2> res_otab;
    pv_pool::Slot &slot(int32_t i) const { return p->slots[(size_t)slots[i]]; }
};

// 1. the arguments
static int pool_feed_check(const PoolFeed &f) {
    const pv_pool *p = f.p;
    const PoolCall &io = f.io;
    if (!p || f.count < 0 || (f.count > 0 && (!f.slots || !f.n || (io.device && !io.out_frames)))) return PV_ERR_INVALID_ARG;
    if (p->poisoned) {
        g_last_error = "pool unusable after an earlier failure: " + p->poison_reason;
        return p->poisoned;
    }
    const int C = p->core.C;
    std::vector<char> seen((size_t)p->cap, 0);
    for (int32_t i = 0; i < f.count; ++i) {
        const int32_t s = f.slots[i], n = f.n[i];
        const char *bad = !pool_slot_ok(p, s) ? "is not open" : seen[(size_t)s] ? "is listed twice" : n < 0 ? "has a negative size" : nullptr;
        if (!bad && io.device) {
            const pv_pool::Slot &sl = p->slots[(size_t)s];
            if (!sl.outq.empty() && sl.outq[0].size() > sl.outq_head)
                bad = "still holds output of pv_pool_feed: retrieve it first";
            else if (n > io.in_pitch) bad = "has more frames than the input pitch";
            else if (n > 0 && !io.d_in) bad = "has no input";
        } else if (!bad && n > 0) {
            if (!io.in) bad = "has no input";
            else
                for (int ch = 0; ch < C && !bad; ++ch)
                    if (!io.in[(size_t)i * C + ch]) bad = "has no input";
        }
        if (bad) {
            g_last_error = "stream pool: slot " + std::to_string(s) + " " + bad;
            return PV_ERR_INVALID_ARG;
        }
        seen[(size_t)s] = 1;
    }
    return PV_OK;
}

// 2. plan every slot; all or nothing: a refusal puts every planner back and leaves the caller's out_frames as it was
static int pool_feed_plan(PoolFeed &f) {
    const PoolCall &io = f.io;
    const int32_t count = f.count;
    f.fresh.resize((size_t)count);
    std::vector<Planner::State> before((size_t)count);
    auto undo = [&](int32_t upto) {
        for (int32_t j = 0; j <= upto; ++j) f.slot(j).planner->restore(before[(size_t)j]);
    };
    for (int32_t i = 0; i < count; ++i) {
        Planner &pl = *f.slot(i).planner;
        before[(size_t)i] = pl.save();
        const int st = pl.feed(f.n[i], f.fresh[(size_t)i]);
        if (st != PV_OK) {
            undo(i);
            g_last_error = "stream pool: slot " + std::to_string(f.slots[i]) + ": " +
                           (g_last_error.empty() ? std::string(plan_reason()) : g_last_error);
            return st;
        }
    }
    // the device feed delivers everything the call makes available (nothing was pending before it: checked above);
    // the retrieve is booked now, the samples follow in stream order
    // (every count is checked before the first is written)
    for (int32_t i = 0; i < count && io.device; ++i) {
        const int32_t got = f.slot(i).planner->available();
        if (got > io.out_pitch || (got > 0 && !io.d_out)) {
            undo(count - 1);
            g_last_error = "stream pool: slot " + std::to_string(f.slots[i]) +
                           (got > io.out_pitch ? " returns " + std::to_string(got) + " frames, more than the output pitch"
                                               : std::string(" has no output buffer"));
            return PV_ERR_INVALID_ARG;
        }
    }
    for (int32_t i = 0; i < count && io.device; ++i) {
        Planner &pl = *f.slot(i).planner;
        io.out_frames[i] = pl.retrieve(pl.available());
    }
    return PV_OK;
}

// 3. the call's descriptor block.  pv_pool_feed: its own, after every device feed in flight has finished (their
// output and any late error of theirs come first).  pv_pool_feed_device: the ring's next, once the call that used
// it last has finished.
static int pool_feed_take_block(PoolFeed &f) {
    pv_pool *p = f.p;
    int st;
    f.blk = &p->sync_desc;
    if (!f.io.device) return pool_drain(p);
    if (!p->ring_ready) { // (everything a device feed allocates in the common case, at the first one)
        for (pv_pool::DescBlock &b : p->ring_desc) {
            if ((st = b.h.alloc(256 * 1024)) != PV_OK || (st = b.d.alloc_on(256 * 1024, p->stream)) != PV_OK) return st;
            hipError_t e = hipEventCreateWithFlags(&b.entry, hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&b.done, hipEventDisableTiming);
            if (e != hipSuccess) return hip_fail(e, "descriptor ring events", __LINE__);
        }
        p->ring_ready = true;
    }
    f.blk = &p->ring_desc[p->ring_next];
    p->ring_next = (p->ring_next + 1) % kPoolDescRing;
    if (f.blk->busy) {
        f.blk->busy = false;
        const hipError_t e = hipEventSynchronize(f.blk->done);
        if (e != hipSuccess) return hip_fail(e, "stream pool device feed", __LINE__);
    }
    return PV_OK;
}

// 4. where the call's new samples are read and its output is written.  pv_pool_feed: the samples packed
// [slot][C][n] into the staging buffer (one copy), the output packed [slot][C][cnt] in the mapped host arena.
// pv_pool_feed_device: the caller's buffers as they are (int16 output: packed in a device arena, converted after
// the launches).
static int pool_feed_place(PoolFeed &f) {
    pv_pool *p = f.p;
    const PoolCall &io = f.io;
    const int32_t count = f.count;
    const int C = p->core.C;
    int st;
    f.to_caller = io.device && io.wire == PV_WIRE_F32;
    for (std::vector<int64_t> *v : {&f.stage_off, &f.out_base, &f.out_cnt, &f.k0, &f.call_base}) v->resize((size_t)count);
    for (int32_t i = 0; i < count; ++i) {
        f.stage_off[(size_t)i] = io.device ? (int64_t)i * C * io.in_pitch : (int64_t)f.stage_total;
        f.stage_total += (size_t)C * f.n[i];
        const std::vector<SliceRec> &fr = f.fresh[(size_t)i];
        f.out_base[(size_t)i] = f.to_caller ? (int64_t)i * C * io.out_pitch : (int64_t)f.out_total;
        f.out_cnt[(size_t)i] = fr.empty() ? 0 : fr.back().K0 + fr.back().cnt - fr.front().K0;
        f.k0[(size_t)i] = fr.empty() ? 0 : fr.front().K0;
        f.out_total += (size_t)C * f.out_cnt[(size_t)i];
        f.groups = std::max(f.groups, (int)((fr.size() + kStreamChunk - 1) / kStreamChunk));
        f.call_base[(size_t)i] = f.slot(i).fed;
    }
    f.ingest_src = io.d_in;
    f.launch_out = static_cast<float *>(io.d_out);
    if (io.device) {
        if (f.to_caller) return PV_OK;
        if (f.out_total > p->d_arena.n) {
            // (the calls in flight still use the old arena)
            const hipError_t e = hipStreamSynchronize(p->stream);
            if (e != hipSuccess) return hip_fail(e, "stream pool device feed", __LINE__);
            if ((st = grow(p->d_arena, f.out_total, 1 << 16, p->stream)) != PV_OK) return st;
        }
        f.launch_out = p->d_arena.p;
        return PV_OK;
    }
    if (f.stage_total > p->h_stage.n) {
        if ((st = grow(p->h_stage, f.stage_total, 1 << 16)) != PV_OK) return st;
#ifdef PV_POOL_MAPPED_INGEST // (measurement build: the ingest kernel reads the page-locked staging over the bus)
        void *sp = nullptr;
        const hipError_t e = hipHostGetDevicePointer(&sp, p->h_stage.p, 0);
        if (e != hipSuccess) return hip_fail(e, "staging mapping", __LINE__);
        p->stage_src = static_cast<float *>(sp);
#else
        if ((st = p->d_stage.alloc_on(p->h_stage.n, p->stream)) != PV_OK) return st;
        p->stage_src = p->d_stage.p;
#endif
    }
    for (int32_t i = 0; i < count; ++i)
        for (int ch = 0; ch < C; ++ch)
            if (f.n[i] > 0)
                memcpy(p->h_stage.p + f.stage_off[(size_t)i] + (size_t)ch * f.n[i], io.in[(size_t)i * C + ch],
                       (size_t)f.n[i] * sizeof(float));
    if (f.out_total > p->h_out.n) {
        if ((st = grow(p->h_out, f.out_total, 1 << 16)) != PV_OK) return st;
        void *op = nullptr;
        const hipError_t e = hipHostGetDevicePointer(&op, p->h_out.p, 0);
        if (e != hipSuccess) return hip_fail(e, "output arena mapping", __LINE__);
        p->out_dev = static_cast<float *>(op);
    }
    f.ingest_src = p->stage_src;
    f.launch_out = p->out_dev;
    return PV_OK;
}

// entry i's samples up to `upto`, where the slot's ring does not hold them yet, onto the group's ingest list
static void pool_feed_ingest(PoolFeed &f, int32_t i, int64_t upto, PoolFeed::Group &g) {
    pv_pool::Slot &sl = f.slot(i);
    if (upto <= sl.uploaded) return;
    PoolIngest e{};
    e.src_off = f.stage_off[(size_t)i] + (sl.uploaded - f.call_base[(size_t)i]);
    e.src_pitch = f.io.device ? f.io.in_pitch : f.n[i];
    e.pos = sl.uploaded;
    e.n = (int32_t)(upto - sl.uploaded);
    e.row0 = f.slots[i] * f.p->core.C;
    f.ingest.push_back(e);
    if (e.n > g.max_in) g.max_in = e.n;
    sl.uploaded = upto;
}

// The PoolSlot of entry i for its fresh slices [ta, tb), one launch: its phase increments, run list, run offsets,
// denominators and resampling tiles go into the blob, its generator job, where the slot whispers, onto f.wjobs;
// env_comp is set where the slot runs the formant stage
static PoolSlot pool_describe_slot(PoolFeed &f, int32_t i, int ta, int tb) {
    const pv_pool *p = f.p;
    const Core &c = p->core;
    const int C = c.C, Tn = tb - ta;
    const int32_t s = f.slots[i];
    const std::vector<SliceRec> &fr = f.fresh[(size_t)i];
    pv_pool::Slot &sl = f.slot(i);
    const Derived &sd = *sl.d;
    const int64_t t0 = sl.slices + ta;
    PoolSlot ps{};
    ps.t0 = t0;
    ps.s0 = (int32_t)(t0 % c.TR);
    ps.Tn = Tn;
    ps.row0 = s * C;
    ps.acc_sel = sl.acc_half | (t0 == 0 ? 2 : 0);
    sl.acc_half ^= 1;
    f.pinc.clear();
    for (int t = ta; t < tb; ++t) f.pinc.push_back(fr[(size_t)t].phase_inc);
    ps.pinc_off = f.blob.put(f.pinc);
    f.wden.clear(), f.wden_hi.clear(), f.cs.clear(), f.ro.clear();
    const int64_t ka = fr[(size_t)ta].K0, kb = fr[(size_t)tb - 1].K0 + fr[(size_t)tb - 1].cnt;
    sl.chain->begin_launch(fr[(size_t)ta]);
    for (int t = ta; t < tb; ++t) sl.chain->add(fr[(size_t)t], INT64_MAX, f.wden, f.wden_hi);
    sl.chain->end_launch(1, f.cs, f.ro); // (one run)
    finish_wden(f.wden, sl.fast);
    ps.cs_off = f.blob.put(f.cs);
    const int32_t ro4[4] = {0, (int32_t)f.cs.size(), 0, 0};
    ps.ro_off = f.blob.put(ro4, sizeof ro4);
    ps.wden_off = f.blob.put(f.wden);
    f.res_tiles.clear(), f.res_otab.clear();
    if (sd.resample && kb > ka) build_res_tiles_of(sd, ka, kb, f.res_tiles, f.res_otab);
    ps.res_ntiles = (int32_t)f.res_tiles.size();
    ps.res_off = f.blob.put(f.res_tiles);
    ps.otab_off = f.blob.put(f.res_otab);
    ps.out_off = f.out_base[(size_t)i] + (ka - f.k0[(size_t)i]);
    ps.out_stride_row = f.to_caller ? f.io.out_pitch : f.out_cnt[(size_t)i];
    ps.k_base = ka;
    ps.wh_off = -1;
    if (sl.voice == PV_VOICE_WHISPER) {
        // the slot's draws of this launch, in the reference's order: slice-major, channel, bins 0 .. hs.  A
        // stream's first launch starts from the pool's fresh state, every later one from the slot's own row
        WhisperJob wj{};
        wj.src_off = (int64_t)(t0 == 0 ? p->cap : s) * kWhisperStatePitch;
        wj.dst_off = (int64_t)s * kWhisperStatePitch;
        wj.out_off = ps.wh_off = (int64_t)s * (int64_t)pool_wphase_stride(p);
        wj.count = (int64_t)Tn * C * (sd.hs + 1);
        wj.per = sd.hs + 1, wj.pitch = c.HP;
        f.wjobs.push_back(wj);
    }
    ps.car_off = -1;
    if (sl.carrier != PV_CARRIER_NONE) {
        // the carrier's frames of this launch lie at the ring positions of the input's: samples up to the last
        // frame's end, from where the slot's row holds them (a restored slot's: from this launch's first frame)
        ps.car_off = (int64_t)s * c.TR * c.HP;
        const int64_t from = std::max(sl.car_pos, t0 * (int64_t)sd.hop), upto = (t0 + Tn - 1) * (int64_t)sd.hop + sd.N;
        if (upto > from) {
            f.cjobs.push_back(carrier_job(p->ctab, sl.carrier == PV_CARRIER_CHORD, from, (int32_t)(upto - from),
                                          (int64_t)s * p->ring, (uint32_t)(from & (int64_t)(p->ring - 1))));
            sl.car_pos = upto;
        }
        PoolSlot cs = ps;
        cs.row0 = s;
        f.car_table.push_back(cs);
        if (p->mixed) f.car_params.push_back(slot_params(sd, 0, 0, nullptr, 0));
    }
    if (sl.fx_on) {
        const float env_comp = formant_env_comp_of(sd.pitch_scale, sl.fx_semitones);
        if (env_comp != 1.0f) ps.env_comp = env_comp; // (as mode FORMANT_CEPSTRAL skips the stage at pitch scale 1)
    }
    return ps;
}

// 5. the descriptors of every group: per group its PoolSlot table and ingest list (a mixed pool: sorted by variant,
// with the PoolParams table), per slot what pool_describe_slot writes; then the egress list, and all of it into the
// call's block
static int pool_feed_describe(PoolFeed &f) {
    pv_pool *p = f.p;
    const Core &c = p->core;
    const int32_t count = f.count;
    int st;
    f.grp.assign((size_t)f.groups + 1, PoolFeed::Group());
    std::vector<PoolSlot> table, fx_table;
    std::vector<PoolParams> params;
    std::vector<int> vkey;
    for (int32_t i = 0; i < count; ++i) f.slot(i).fed += f.n[i];
    for (int gi = 0; gi < f.groups; ++gi) {
        PoolFeed::Group &g = f.grp[(size_t)gi];
        table.clear(), fx_table.clear(), params.clear(), vkey.clear();
        f.wjobs.clear(), f.ingest.clear();
        f.cjobs.clear(), f.car_table.clear(), f.car_params.clear();
        for (int32_t i = 0; i < count; ++i) {
            const int nf = (int)f.fresh[(size_t)i].size(), ta = gi * kStreamChunk;
            if (nf <= ta) continue;
            const int tb = nf - ta < kStreamChunk ? nf : ta + kStreamChunk;
            const pv_pool::Slot &sl = f.slot(i);
            const Derived &sd = *sl.d;
            int64_t need = (sl.slices + tb - 1) * (int64_t)sd.hop + sd.N;
            if (need > sl.fed) need = sl.fed;
            pool_feed_ingest(f, i, need, g);
            const PoolSlot ps = pool_describe_slot(f, i, ta, tb);
            if (ps.env_comp != 0.f) { // (the formant stage is on for the slot)
                fx_table.push_back(ps);
                if (ps.Tn > g.fx_max_tn) g.fx_max_tn = ps.Tn;
            }
            table.push_back(ps);
            if (ps.Tn > g.max_tn) g.max_tn = ps.Tn;
            if (ps.res_ntiles > g.max_tiles) g.max_tiles = ps.res_ntiles;
            if (p->mixed) {
                params.push_back(slot_params(sd, sl.tab_bytes, sl.lds_floats,
                                             sd.resample ? p->d_tabs.p + (size_t)sl.tab * p->tab_stride : nullptr,
                                             (size_t)(p->max_sinc + 3) / 4));
                vkey.push_back(variant_key(sd, sl.fast));
            }
        }
        if (p->mixed && !table.empty()) {
            // slots of one variant contiguous (stable: the same order as the call lists them otherwise)
            std::vector<int> ord(table.size());
            for (size_t k = 0; k < ord.size(); ++k) ord[k] = (int)k;
            std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return vkey[(size_t)x] < vkey[(size_t)y]; });
            std::vector<PoolSlot> t2(table.size());
            std::vector<PoolParams> q2(table.size());
            for (size_t k = 0; k < ord.size(); ++k) {
                t2[k] = table[(size_t)ord[k]];
                q2[k] = params[(size_t)ord[k]];
                variant_runs_add(g.vr, (int)k, vkey[(size_t)ord[k]], t2[k].res_ntiles, q2[k].lds_floats, q2[k].tab_bytes, 1);
            }
            table.swap(t2);
            params.swap(q2);
            g.params_off = f.blob.put(params);
        }
        g.nslots = (int)table.size();
        g.table_off = f.blob.put(table);
        g.fx_nslots = (int)fx_table.size();
        g.fx_off = f.blob.put(fx_table);
        g.nwj = (int)f.wjobs.size();
        g.wj_off = f.blob.put(f.wjobs);
        f.any_whisper = f.any_whisper || !f.wjobs.empty();
        g.ncj = (int)f.cjobs.size();
        g.cj_off = f.blob.put(f.cjobs);
        for (const CarrierJob &cj : f.cjobs) g.max_cn = std::max(g.max_cn, (int)cj.n);
        g.car_nslots = (int)f.car_table.size();
        g.car_off = f.blob.put(f.car_table);
        g.car_params_off = f.blob.put(f.car_params);
        for (const PoolSlot &cs : f.car_table) g.car_max_tn = std::max(g.car_max_tn, (int)cs.Tn);
        f.any_carrier = f.any_carrier || !f.car_table.empty();
        g.ningest = (int)f.ingest.size();
        g.ingest_off = f.blob.put(f.ingest);
    }
    PoolFeed::Group &last = f.grp[(size_t)f.groups];
    f.ingest.clear();
    for (int32_t i = 0; i < count; ++i) pool_feed_ingest(f, i, f.slot(i).fed, last);
    last.ningest = (int)f.ingest.size();
    last.ingest_off = f.blob.put(f.ingest);
    for (int32_t i = 0; i < count; ++i) {
        pv_pool::Slot &sl = f.slot(i);
        const int64_t nf = (int64_t)f.fresh[(size_t)i].size();
        sl.slices += nf;
        if (nf > 0) sl.tap_n = (int)std::min<int64_t>(nf, c.TR);
    }
    if (f.io.device && !f.to_caller) {
        std::vector<PoolEgress> eg;
        for (int32_t i = 0; i < count; ++i) {
            const int64_t cnt = f.out_cnt[(size_t)i];
            if (cnt <= 0) continue;
            eg.push_back(PoolEgress{f.out_base[(size_t)i], cnt, (int64_t)i * c.C * f.io.out_pitch, f.io.out_pitch, (int32_t)cnt, 0});
            if (cnt > f.max_egress) f.max_egress = (int)cnt;
        }
        f.negress = (int)eg.size();
        f.egress_off = f.blob.put(eg);
    }
    if (f.any_carrier) f.ctab_off = f.blob.put(p->ctab.v);
    pv_pool::DescBlock *blk = f.blk;
    const size_t bytes = f.blob.bytes.size();
    if (bytes > blk->h.n)
        if ((st = grow(blk->h, bytes, 256 * 1024)) != PV_OK || (st = blk->d.alloc_on(blk->h.n, p->stream)) != PV_OK) return st;
    memcpy(blk->h.p, f.blob.bytes.data(), bytes);
    if (f.any_carrier && (st = pool_carrier_buffers(p)) != PV_OK) return st;
    return f.any_whisper ? pool_voice_buffers(p) : PV_OK;
}

// A launch group's carrier slots: one launch writes every slot's new carrier samples into its row of the carrier ring,
// one launch of the set's analysis kernel turns the carrier frames of the group's slices into the slots' carrier planes
// (find_peaks = 0, one row per slot: as Core::launch_chunk analyses a batch's carrier row).
static int pool_launch_carrier(const pv_pool *p, int64_t cj_off, int ncj, int max_cn, int64_t car_off, int car_nslots,
                               int car_max_tn, int64_t car_params_off, const char *d_desc, int64_t ctab_off, float *out,
                               int *nlaunch) {
    const Core &c = p->core;
    CarrierArgs ga{};
    ga.out = p->d_cring.p;
    ga.tab = reinterpret_cast<const float *>(d_desc + ctab_off);
    for (int k = 0; k < kCarrierTabs; ++k) ga.off[k] = p->ctab.off[k], ga.len[k] = p->ctab.len[k];
    ga.mask = (uint32_t)(p->ring - 1);
    ga.jobs = reinterpret_cast<const CarrierJob *>(d_desc + cj_off);
    if (ncj > 0 && max_cn > 0) {
        launch_carrier(ga, ncj, max_cn, p->stream);
        ++*nlaunch;
        const hipError_t ge = hipGetLastError();
        if (ge != hipSuccess) return hip_fail(ge, "carrier generator launch", __LINE__);
    }
    AnalyzeArgs aa = c.analyze_args(c.C);
    aa.rows = 1;
    aa.find_peaks = 0;
    aa.mag = p->d_cmag.p;
    aa.phase = p->d_cphase.p;
    aa.ia = InAddr{};
    aa.ia.in = p->d_cring.p;
    aa.ia.stride_c = p->ring;
    aa.ia.stride_s = p->ring;
    aa.ia.mask = (uint64_t)(p->ring - 1);
    aa.ia.len = INT64_MAX;
    const PoolLaunch pl{reinterpret_cast<const PoolSlot *>(d_desc + car_off), d_desc, out, car_nslots, car_max_tn, 0};
    const LaunchCheck lc{"pool", "stream pool: no per-slot ", nlaunch, true};
    const bool ok = p->mixed ? launch_pmix_analyze(aa, pl, reinterpret_cast<const PoolParams *>(d_desc + car_params_off), p->stream)
                             : launch_pool_analyze(aa, pl, p->stream);
    return lc.after(ok, "carrier analysis");
}

// 6. the copies and the launches.  pv_pool_feed: the previous call has finished with both staging buffers.
// pv_pool_feed_device: the pool's stream first waits for what the caller's stream holds now (the producer of d_in,
// the last reader of d_out), and the caller's stream then for the block's event behind the launches.
static int pool_feed_enqueue(PoolFeed &f) {
    pv_pool *p = f.p;
    const Core &c = p->core;
    const PoolCall &io = f.io;
    pv_pool::DescBlock *blk = f.blk;
    char *const d_desc = blk->d.p;
    int st;
    hipError_t ce = hipSuccess;
    if (io.device) {
        ce = hipEventRecord(blk->entry, io.user);
        if (ce == hipSuccess) ce = hipStreamWaitEvent(p->stream, blk->entry, 0);
        if (ce != hipSuccess) return hip_fail(ce, "stream pool entry event", __LINE__);
    }
#ifndef PV_POOL_MAPPED_INGEST
    if (f.stage_total && !io.device)
        ce = hipMemcpyAsync(p->d_stage.p, p->h_stage.p, f.stage_total * sizeof(float), hipMemcpyHostToDevice, p->stream);
    if (ce != hipSuccess) return hip_fail(ce, "input upload", __LINE__);
#endif
    ce = hipMemcpyAsync(d_desc, blk->h.p, f.blob.bytes.size(), hipMemcpyHostToDevice, p->stream);
    if (ce != hipSuccess) return hip_fail(ce, "descriptor upload", __LINE__);
    int nlaunch = 0;
    const int cm = phase_mode(c.d);
    for (int gi = 0; gi <= f.groups; ++gi) {
        const PoolFeed::Group &g = f.grp[(size_t)gi];
        launch_pool_ingest(f.ingest_src, io.wire, p->d_in.p, p->ring, c.C, reinterpret_cast<const PoolIngest *>(d_desc + g.ingest_off),
                           g.ningest, g.max_in, p->stream);
        if (g.ningest > 0 && g.max_in > 0) ++nlaunch;
        const hipError_t ie = hipGetLastError();
        if (ie != hipSuccess) return hip_fail(ie, "input ingest", __LINE__);
        if (gi == f.groups || g.nslots == 0) continue;
        auto table_at = [&](int64_t off) { return reinterpret_cast<const PoolSlot *>(d_desc + off); };
        const PoolLaunch pl{table_at(g.table_off), d_desc, f.launch_out, g.nslots, g.max_tn, g.max_tiles};
        const PoolLaunch fx{table_at(g.fx_off), d_desc, f.launch_out, g.fx_nslots, g.fx_max_tn, g.max_tiles};
        const PoolLaunch *const fxp = g.fx_nslots > 0 ? &fx : nullptr;
        const float *whisper = nullptr;
        if (g.nwj > 0) { // the group's whisper slots draw their phases: one launch, one wave per slot
            launch_whisper(p->d_wstate.p, p->d_wphase.p, reinterpret_cast<const WhisperJob *>(d_desc + g.wj_off), g.nwj,
                           p->mixed ? PV_CENSUS_SET_PMIX : PV_CENSUS_SET_POOL, c.d.fft.nc, p->stream);
            ++nlaunch;
            const hipError_t we = hipGetLastError();
            if (we != hipSuccess) return hip_fail(we, "voice generator launch", __LINE__);
            whisper = p->d_wphase.p;
        }
        PoolCarrier car{};
        if (g.car_nslots > 0) { // the group's carrier slots: their carrier samples, then the planes of its frames
            if ((st = pool_launch_carrier(p, g.cj_off, g.ncj, g.max_cn, g.car_off, g.car_nslots, g.car_max_tn,
                                          g.car_params_off, d_desc, f.ctab_off, f.launch_out, &nlaunch)) != PV_OK)
                return st;
            car.cmag = p->d_cmag.p, car.cphase = p->d_cphase.p;
        }
        if (p->mixed) {
            const PoolParams *q = reinterpret_cast<const PoolParams *>(d_desc + g.params_off);
            if ((st = pool_mix_launch_group(p, pl, q, g.vr, &nlaunch, fxp, whisper, car)) != PV_OK) return st;
        } else {
            if ((st = pool_launch_group(p, pl, true, fxp, whisper, car)) != PV_OK) return st;
            nlaunch += 2 + (cm == 0 || cm == 1 ? 1 : 0) + (c.d.resample && pl.max_tiles > 0 ? 1 : 0) + (fxp ? 1 : 0);
        }
    }
    if (f.negress > 0) { // int16: the arena into the caller's buffer

        launch_pool_egress_i16(p->d_arena.p, static_cast<int16_t *>(io.d_out), c.C,
                               reinterpret_cast<const PoolEgress *>(d_desc + f.egress_off), f.negress, f.max_egress, p->stream);
        ++nlaunch;
        const hipError_t ee = hipGetLastError();
        if (ee != hipSuccess) return hip_fail(ee, "int16 egress", __LINE__);
    }
    p->last_launches = nlaunch;
    if (!io.device) return PV_OK;
    // the block's event behind the launches, which the caller's stream waits for
    ce = hipEventRecord(blk->done, p->stream);
    if (ce == hipSuccess) {
        blk->busy = true;
        ce = hipStreamWaitEvent(io.user, blk->done, 0);
    }
    if (ce != hipSuccess) return hip_fail(ce, "stream pool exit event", __LINE__);
    p->last_host_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - f.t_call).count();
    p->last_wait_us = 0;
    return PV_OK;
}

// 7. wait (pv_pool_feed): a sequence number behind the launches, spun on with a wall-clock bound (or a stream
// synchronisation where the device has no stream memory operations)
static int pool_feed_wait(PoolFeed &f) {
    pv_pool *p = f.p;
    hipError_t he = hipSuccess;
    const auto t_wait = std::chrono::steady_clock::now();
    if (p->wait_value) {
        const uint32_t seq = ++p->flag_seq;
        he = hipStreamWriteValue32(p->stream, p->flag_dev, seq, 0);
        if (he == hipSuccess) {
            volatile uint32_t *fl = p->h_flag.p;
            const auto t_start = std::chrono::steady_clock::now();
            uint32_t spins = 0;
            while (__atomic_load_n(fl, __ATOMIC_ACQUIRE) != seq) {
                if ((++spins & 0xfffu) != 0) continue;
                const hipError_t q = hipStreamQuery(p->stream);
                if (q != hipSuccess && q != hipErrorNotReady) {
                    he = q;
                    break;
                }
                if (__atomic_load_n(fl, __ATOMIC_ACQUIRE) == seq) break;
                if (std::chrono::steady_clock::now() - t_start > std::chrono::seconds(10)) {
                    g_last_error = "stream pool: the call's kernels did not finish within 10 s";
                    return PV_ERR_HIP;
                }
            }
        }
    } else {
        he = hipStreamSynchronize(p->stream);
    }
    if (he == hipSuccess) he = hipGetLastError();
    if (he != hipSuccess) return hip_fail(he, "stream pool call", __LINE__);
    p->last_wait_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_wait).count();
    p->last_host_us = std::chrono::duration<double, std::micro>(t_wait - f.t_call).count();
    return PV_OK;
}

// 8. deliver (pv_pool_feed): the arena into the slots' FIFOs
static void pool_feed_deliver(PoolFeed &f) {
    const int C = f.p->core.C;
    for (int32_t i = 0; i < f.count; ++i) {
        const int64_t cnt = f.out_cnt[(size_t)i];
        if (cnt <= 0) continue;
        pv_pool::Slot &sl = f.slot(i);
        for (int ch = 0; ch < C; ++ch) {
            const float *src = f.p->h_out.p + f.out_base[(size_t)i] + (size_t)ch * cnt;
            sl.outq[(size_t)ch].insert(sl.outq[(size_t)ch].end(), src, src + cnt);
        }
    }
}

// A feed in its phases.  1 and 2 refuse and leave the pool as it was.  From hipSetDevice on, device state and host
// bookkeeping move together: a phase that fails there poisons the pool.
static int pool_feed(pv_pool *p, int32_t count, const int32_t *slots, const int32_t *n, const PoolCall &io) {
    g_last_error.clear();
    plan_reason_clear();
    PoolFeed f{p, count, slots, n, io};
    int st;
    if ((st = pool_feed_check(f)) != PV_OK) return st;
    p->last_launches = 0;
    if (count == 0) return PV_OK;
    f.t_call = std::chrono::steady_clock::now();
    if ((st = pool_feed_plan(f)) != PV_OK) return st;
    const hipError_t e = hipSetDevice(p->core.device);
    st = e == hipSuccess ? PV_OK : hip_fail(e, "hipSetDevice", __LINE__);
    if (st == PV_OK) st = pool_feed_take_block(f);
    if (st == PV_OK) st = pool_feed_place(f);
    if (st == PV_OK) st = pool_feed_describe(f);
    if (st == PV_OK) st = pool_feed_enqueue(f);
    if (st == PV_OK && !io.device) st = pool_feed_wait(f);
    if (st != PV_OK) {
        p->poisoned = st;
        p->poison_reason = g_last_error.empty() ? pv_strerror(st) : g_last_error;
        return st;
    }
    if (!io.device) pool_feed_deliver(f);
    return PV_OK;
}

int pv_pool_feed(pv_pool *p, int32_t count, const int32_t *slots, const float *const *in, const int32_t *n) {
    PoolCall io;
    io.in = in;
    return pool_feed(p, count, slots, n, io);
}

int pv_pool_feed_device(pv_pool *p, int32_t count, const int32_t *slots, const int32_t *n, const void *d_in,
                        int64_t in_pitch, void *d_out, int64_t out_pitch, int32_t wire, int32_t *out_frames,
                        void *hip_stream) {
    if (p && (wire != PV_WIRE_F32 && wire != PV_WIRE_I16)) {
        g_last_error = "stream pool: unknown wire " + std::to_string(wire);
        return PV_ERR_INVALID_ARG;
    }
    if (p && (in_pitch < 0 || out_pitch < 0)) {
        g_last_error = "stream pool: negative pitch";
        return PV_ERR_INVALID_ARG;
    }
    PoolCall io;
    io.device = true;
    io.d_in = d_in, io.d_out = d_out;
    io.in_pitch = in_pitch, io.out_pitch = out_pitch;
    io.wire = wire;
    io.user = static_cast<hipStream_t>(hip_stream);
    io.out_frames = out_frames;
    return pool_feed(p, count, slots, n, io);
}

int pv_pool_plan_feed(pv_pool *p, int32_t count, const int32_t *slots, const int32_t *n, int32_t *out_frames) {
    g_last_error.clear();
    plan_reason_clear();
    if (!p || count < 0 || (count > 0 && (!slots || !n || !out_frames))) return PV_ERR_INVALID_ARG;
    for (int32_t i = 0; i < count; ++i)
        if (!pool_slot_ok(p, slots[i]) || n[i] < 0) {
            g_last_error = "stream pool: slot " + std::to_string(slots[i]) + (n[i] < 0 ? " has a negative size" : " is not open");
            return PV_ERR_INVALID_ARG;
        }
    std::vector<SliceRec> scratch;
    std::vector<int32_t> frames((size_t)count); // (written to the caller's array only when every slot has planned)
    for (int32_t i = 0; i < count; ++i) {
        Planner &pl = *p->slots[(size_t)slots[i]].planner;
        const Planner::State before = pl.save();
        scratch.clear();
        const int st = pl.feed(n[i], scratch);
        frames[(size_t)i] = pl.available();
        pl.restore(before);
        if (st != PV_OK) {
            g_last_error = "stream pool: slot " + std::to_string(slots[i]) + ": " +
                           (g_last_error.empty() ? std::string(plan_reason()) : g_last_error);
            return st;
        }
    }
    for (int32_t i = 0; i < count; ++i) out_frames[i] = frames[(size_t)i];
    return PV_OK;
}

// ---------------------------------------------------------------- stream pool snapshots
static int64_t pool_slot_pending(const pv_pool::Slot &sl) {
    return sl.outq.empty() ? 0 : (int64_t)(sl.outq[0].size() - sl.outq_head);
}
// the header of the slot's blob as pv_pool_save would write it now, sizes included (the host state itself:
// snap::encode_head)
static void pool_snap_header(const pv_pool *p, const pv_pool::Slot &sl, snap::Header &h) {
    h = snap::Header{};
    pool_snap_geometry(p, h);
    h.time_ratio = sl.d->cfg.time_ratio;
    h.pitch_semitones = sl.d->cfg.pitch_semitones;
    if (sl.voice == PV_VOICE_WHISPER) h.mode = PV_MODE_WHISPER; // (the stream is that engine's: a version-2 blob)
    if (sl.carrier != PV_CARRIER_NONE) h.mode = carrier_mode(sl.carrier); // (... a vocoder engine's: version 3)
    snap::fill_sizes(h, (int32_t)sl.chain->live.size(), pool_slot_pending(sl));
}
// the first field in which a blob's pool differs from this one (nullptr: none).  Both sides are pools' own derived
// values, not creation arguments.
static const char *pool_snap_mismatch(const snap::Header &blob, const snap::Header &pool) {
#define PV_SNAP_FIELD(f, name) \
    if (blob.f != pool.f) return name
    PV_SNAP_FIELD(sample_rate, "sample rate");
    PV_SNAP_FIELD(channels, "channels");
    // (the voice and carrier settings: such a stream lives in a ROBOTIC pool)
    if ((blob.mode == PV_MODE_WHISPER || carrier_of_mode(blob.mode) != PV_CARRIER_NONE ? PV_MODE_ROBOTIC : blob.mode) != pool.mode)
        return "mode";
    PV_SNAP_FIELD(coremode, "coremode");
    PV_SNAP_FIELD(N, "FFT size");
    PV_SNAP_FIELD(hopsize, "hop setting");
    PV_SNAP_FIELD(arith, "arithmetic setting");
    PV_SNAP_FIELD(phase_stage, "phase stage");
    PV_SNAP_FIELD(hs, "half spectrum");
    PV_SNAP_FIELD(ring, "input-ring length");
    PV_SNAP_FIELD(TR, "plane-ring slots (TR)");
    PV_SNAP_FIELD(HP, "plane pitch (HP)");
    PV_SNAP_FIELD(PKP, "peak-list pitch (PKP)");
    PV_SNAP_FIELD(AR, "accumulator-ring length");
    PV_SNAP_FIELD(stream_len, "stream-ring length");
#undef PV_SNAP_FIELD
    return nullptr;
}

// room for a call's staging (device and page-locked image) and segment table; a failed allocation leaves the pool as
// usable as it was
static int pool_snap_reserve(pv_pool *p, size_t stage_bytes, size_t nsegs) {
    int st;
    if (stage_bytes > p->d_snap.n || stage_bytes > p->h_snap.n) {
        if ((st = grow(p->d_snap, stage_bytes, (size_t)1 << 20, p->stream)) != PV_OK) {
            p->d_snap.release();
            return st;
        }
        if ((st = p->h_snap.alloc(p->d_snap.n)) != PV_OK) {
            p->h_snap.n = 0;
            return st;
        }
    }
    if (nsegs > p->h_seg.n || !p->seg_dev) {
        p->seg_dev = nullptr;
        if ((st = grow(p->h_seg, nsegs, 256)) != PV_OK) {
            p->h_seg.n = 0;
            return st;
        }
        void *dp = nullptr;
        HIPC(hipHostGetDevicePointer(&dp, p->h_seg.p, 0));
        p->seg_dev = static_cast<const SnapSeg *>(dp);
    }
    return PV_OK;
}

// The call's segment table: entry i of `slot_of` is staged at i * snap::device_bytes(h), its buffers in directory
// order, each padded to 16 bytes -- a blob's payload as it is.  Returns the number of segments; *parts: workgroups per
// segment (about 64 KB each, and about 4096 workgroups in all at the most).
// (hd[i]: blob i's header -- a whisper slot's payload has one segment more; stage_off[i]: where it is staged)
static int pool_snap_table(pv_pool *p, const std::vector<snap::Header> &hd, const std::vector<int32_t> &slot_of,
                           const std::vector<int64_t> &stage_off, int *parts) {
    int n = 0;
    int64_t largest = 0;
    for (size_t i = 0; i < slot_of.size(); ++i) {
        const snap::Header &h = hd[i];
        int64_t off = stage_off[i];
        for (int b = 0; b < snap::kBufCount; ++b)
            if (const int64_t per = snap::seg_bytes(h, b)) {
                p->h_seg.p[n++] = SnapSeg{b, 0, (int64_t)slot_of[i] * per, off, per};
                off += snap::pad16(per);
                if (per > largest) largest = per;
            }
    }
    int w = (int)std::min<int64_t>(64, (largest + 65535) / 65536);
    while (w > 1 && (int64_t)w * n > 4096) w /= 2;
    *parts = w < 1 ? 1 : w;
    return n;
}
static SnapArgs pool_snap_args(const pv_pool *p, bool to_stage) {
    SnapArgs a{};
    for (int b = 0; b < snap::kBufCount; ++b) {
        size_t have;
        a.bufs[b] = b == snap::kBufWhisper ? reinterpret_cast<char *>(p->d_wstate.p) : pool_snap_buffer(p, b, &have);
    }
    a.segs = p->seg_dev;
    a.stage = p->d_snap.p;
    a.to_stage = to_stage ? 1 : 0;
    return a;
}
static_assert(snap::kBufCount <= kSnapBufs, "SnapArgs holds every buffer of a blob");

// where each blob's device payload is staged, one behind the other; returns the total
static int64_t pool_snap_stage_layout(const std::vector<snap::Header> &hd, std::vector<int64_t> &stage_off) {
    int64_t total = 0;
    stage_off.clear();
    for (const snap::Header &h : hd) {
        stage_off.push_back(total);
        total += snap::device_bytes(h);
    }
    return total;
}
static bool pool_snap_any_voice(const std::vector<snap::Header> &hd) {
    for (const snap::Header &h : hd)
        if (h.mode == PV_MODE_WHISPER) return true;
    return false;
}

int64_t pv_pool_snapshot_bytes(const pv_pool *p, int32_t slot) {
    if (!pool_slot_ok(p, slot)) return -1;
    snap::Header h;
    pool_snap_header(p, p->slots[(size_t)slot], h);
    return (int64_t)h.total_bytes;
}

int pv_pool_save(pv_pool *p, int32_t count, const int32_t *slots, void *const *blobs, const int64_t *capacity,
                 int64_t *bytes) {
    g_last_error.clear();
    plan_reason_clear();
    if (!p || count < 0 || (count > 0 && (!slots || !blobs || !capacity || !bytes))) {
        g_last_error = "stream pool save: a NULL argument";
        return PV_ERR_INVALID_ARG;
    }
    if (p->poisoned) {
        g_last_error = "pool unusable after an earlier failure: " + p->poison_reason;
        return p->poisoned;
    }
    Core &c = p->core;
    std::vector<snap::Header> hd((size_t)count);
    {
        std::vector<char> seen((size_t)p->cap, 0);
        for (int32_t i = 0; i < count; ++i) {
            const int32_t s = slots[i];
            std::string bad = !pool_slot_ok(p, s) ? "is not open" : seen[(size_t)s] ? "is listed twice" : !blobs[i] ? "has no blob" : "";
            if (bad.empty()) {
                pool_snap_header(p, p->slots[(size_t)s], hd[(size_t)i]);
                if (capacity[i] < (int64_t)hd[(size_t)i].total_bytes)
                    bad = "needs " + std::to_string(hd[(size_t)i].total_bytes) + " bytes, the blob has " + std::to_string(capacity[i]);
            }
            if (!bad.empty()) {
                g_last_error = "stream pool save: slot " + std::to_string(s) + " " + bad;
                return PV_ERR_INVALID_ARG;
            }
            seen[(size_t)s] = 1;
        }
    }
    if (count == 0) return PV_OK;
    int st;
    if ((st = pool_snap_check_buffers(p, hd[0])) != PV_OK) return st;
    HIPC(hipSetDevice(c.device));
    if ((st = pool_drain(p)) != PV_OK) return st; // (the device feeds in flight come first, as for pv_pool_feed)
    std::vector<int64_t> stage_off;
    const int64_t dev_total = pool_snap_stage_layout(hd, stage_off);
    if ((st = pool_snap_reserve(p, (size_t)dev_total, (size_t)count * snap::kBufCount)) != PV_OK) return st;
    if (pool_snap_any_voice(hd) && (st = pool_voice_buffers(p)) != PV_OK) return st;
    auto fail = [&](int code) {
        p->poisoned = code;
        p->poison_reason = g_last_error.empty() ? pv_strerror(code) : g_last_error;
        return code;
    };
    int parts = 1;
    const int nsegs = pool_snap_table(p, hd, std::vector<int32_t>(slots, slots + count), stage_off, &parts);
    launch_pool_snapshot(pool_snap_args(p, true), nsegs, parts, p->stream);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(p->h_snap.p, p->d_snap.p, (size_t)dev_total, hipMemcpyDeviceToHost, p->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
    if (e != hipSuccess) return fail(hip_fail(e, "stream pool save", __LINE__));
    p->last_launches = 1;
    for (int32_t i = 0; i < count; ++i) {
        const pv_pool::Slot &sl = p->slots[(size_t)slots[i]];
        snap::Header &h = hd[(size_t)i];
        snap::HostState hs;
        hs.plan = sl.planner->save();
        hs.fed = sl.fed, hs.uploaded = sl.uploaded, hs.slices = sl.slices;
        hs.acc_half = sl.acc_half;
        hs.any_upper_skip = sl.chain->any_upper_skip;
        for (const ChainBuilder::Live &f : sl.chain->live) hs.live.push_back(snap::LiveFrame{f.P, f.flags, 0});
        std::vector<const float *> pend((size_t)c.C, nullptr);
        for (int ch = 0; ch < c.C && !sl.outq.empty(); ++ch) pend[(size_t)ch] = sl.outq[(size_t)ch].data() + sl.outq_head;
        uint8_t *blob = static_cast<uint8_t *>(blobs[i]);
        snap::encode_head(h, hs, pend.data(), pool_slot_pending(sl), blob);
        uint8_t *q = blob + snap::payload_offset(h);
        memcpy(q, p->h_snap.p + (size_t)stage_off[(size_t)i], (size_t)snap::device_bytes(h));
        for (int b = 0; b < snap::kBufCount; ++b) // (the padding between segments is zeros whatever the staging held)
            if (const int64_t per = snap::seg_bytes(h, b)) {
                memset(q + per, 0, (size_t)(snap::pad16(per) - per));
                q += snap::pad16(per);
            }
        snap::seal(blob, h);
    }
    for (int32_t i = 0; i < count; ++i) bytes[i] = (int64_t)hd[(size_t)i].total_bytes;
    return PV_OK;
}

int pv_pool_restore(pv_pool *p, int32_t count, const void *const *blobs, const int64_t *bytes, int32_t *slots) {
    g_last_error.clear();
    plan_reason_clear();
    if (!p || count < 0 || (count > 0 && (!blobs || !bytes || !slots))) {
        g_last_error = "stream pool restore: a NULL argument";
        return PV_ERR_INVALID_ARG;
    }
    if (p->poisoned) {
        g_last_error = "pool unusable after an earlier failure: " + p->poison_reason;
        return p->poisoned;
    }
    if (count == 0) return PV_OK;
    Core &c = p->core;
    // 1. everything that can refuse, on the host: the blobs, the pool's compatibility, the slots' constants, free slots
    std::vector<snap::Header> hd((size_t)count);
    std::vector<std::unique_ptr<Derived>> own((size_t)count);
    snap::Header geo{};
    pool_snap_geometry(p, geo);
    for (int32_t i = 0; i < count; ++i) {
        snap::Header &h = hd[(size_t)i];
        const std::string who = "stream pool restore: blob " + std::to_string(i) + ": ";
        if (const char *why = snap::validate(blobs[i], bytes[i], &h)) {
            g_last_error = who + why;
            return PV_ERR_INVALID_ARG;
        }
        if (const char *field = pool_snap_mismatch(h, geo)) {
            g_last_error = who + "this pool cannot host it: its " + field + " differs";
            return PV_ERR_INVALID_ARG;
        }
        if (!pool_in_range(p->range, h.time_ratio, h.pitch_semitones)) {
            g_last_error = who + (p->mixed ? "its pitch / time ratio lies outside the pool's range"
                                           : "a pool from pv_pool_create takes only its configuration's pitch / time ratio");
            return PV_ERR_INVALID_ARG;
        }
        if (const int carrier = carrier_of_mode(h.mode)) { // a carrier slot's constants are the vocoder engine's
            const int st = pool_carrier_constants(p, h.time_ratio, h.pitch_semitones, carrier, own[(size_t)i]);
            if (st != PV_OK) {
                g_last_error = who + g_last_error;
                return st;
            }
        } else if (p->mixed) {
            const int st = pool_slot_constants(p, h.time_ratio, h.pitch_semitones, own[(size_t)i]);
            if (st != PV_OK) {
                g_last_error = who + g_last_error;
                return st;
            }
        }
    }
    std::vector<int32_t> dst;
    for (int32_t s = 0; s < p->cap && (int32_t)dst.size() < count; ++s)
        if (!p->slots[(size_t)s].open) dst.push_back(s);
    if ((int32_t)dst.size() < count) {
        g_last_error = "stream pool restore: " + std::to_string(count) + " blobs, " + std::to_string(dst.size()) + " free slots";
        return PV_ERR_INVALID_ARG;
    }
    int st;
    if ((st = pool_snap_check_buffers(p, hd[0])) != PV_OK) return st;
    // 2. the device side
    HIPC(hipSetDevice(c.device));
    if ((st = pool_drain(p)) != PV_OK) return st;
    std::vector<int64_t> stage_off; // (a whisper slot's payload has one segment more than a robotic one's)
    const int64_t dev_total = pool_snap_stage_layout(hd, stage_off);
    if ((st = pool_snap_reserve(p, (size_t)dev_total, (size_t)count * snap::kBufCount)) != PV_OK) return st;
    if (pool_snap_any_voice(hd) && (st = pool_voice_buffers(p)) != PV_OK) return st;
    // a mixed pool's table arena, as pv_pool_open_with: each entry is held from here on, so that two blobs of one new
    // ratio share it
    std::vector<int> tab((size_t)count, -1);
    for (int32_t i = 0; i < count; ++i)
        if (own[(size_t)i] && own[(size_t)i]->resample) {
            if ((st = pool_tab_acquire(p, *own[(size_t)i], &tab[(size_t)i])) != PV_OK) {
                for (int32_t j = 0; j < i; ++j)
                    if (tab[(size_t)j] >= 0) --p->tabs[(size_t)tab[(size_t)j]].refs;
                return st;
            }
            ++p->tabs[(size_t)tab[(size_t)i]].refs;
        }
    for (int32_t i = 0; i < count; ++i)
        memcpy(p->h_snap.p + (size_t)stage_off[(size_t)i],
               static_cast<const uint8_t *>(blobs[i]) + snap::payload_offset(hd[(size_t)i]), (size_t)snap::device_bytes(hd[(size_t)i]));
    auto fail = [&](int code) {
        p->poisoned = code;
        p->poison_reason = g_last_error.empty() ? pv_strerror(code) : g_last_error;
        return code;
    };
    int parts = 1;
    const int nsegs = pool_snap_table(p, hd, dst, stage_off, &parts);
    hipError_t e = hipMemcpyAsync(p->d_snap.p, p->h_snap.p, (size_t)dev_total, hipMemcpyHostToDevice, p->stream);
    if (e == hipSuccess) {
        launch_pool_snapshot(pool_snap_args(p, false), nsegs, parts, p->stream);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
    if (e != hipSuccess) return fail(hip_fail(e, "stream pool restore", __LINE__));
    p->last_launches = 1;
    // 3. the slots' host state
    for (int32_t i = 0; i < count; ++i) {
        const snap::Header &h = hd[(size_t)i];
        if (tab[(size_t)i] >= 0) --p->tabs[(size_t)tab[(size_t)i]].refs; // (pool_slot_begin counts it for the slot)
        pool_slot_begin(p, dst[(size_t)i], std::move(own[(size_t)i]), tab[(size_t)i]);
        pv_pool::Slot &sl = p->slots[(size_t)dst[(size_t)i]];
        snap::HostState hs;
        snap::decode_host(blobs[i], h, hs);
        sl.planner->restore(hs.plan);
        for (const snap::LiveFrame &f : hs.live) sl.chain->live.push_back(ChainBuilder::Live{f.P, f.flags});
        sl.chain->any_upper_skip = hs.any_upper_skip;
        sl.fed = hs.fed, sl.uploaded = hs.uploaded, sl.slices = hs.slices;
        sl.tap_n = 0; // (a blob carries the recurrences' state, not the planes of its last launch)
        sl.acc_half = hs.acc_half;
        if (h.mode == PV_MODE_WHISPER) sl.voice = PV_VOICE_WHISPER; // (its state row came with the payload)
        // (a carrier slot's row of the carrier ring is not in the blob: its next launch group rewrites what its frames
        // read, from the closed form -- pool_describe_slot starts at the group's first frame)
        sl.carrier = carrier_of_mode(h.mode);
        for (int ch = 0; ch < c.C && h.pending > 0; ++ch) {
            sl.outq[(size_t)ch].resize((size_t)h.pending);
            memcpy(sl.outq[(size_t)ch].data(), snap::pending_of(blobs[i], h, ch), (size_t)h.pending * sizeof(float));
        }
    }
    for (int32_t i = 0; i < count; ++i) slots[i] = dst[(size_t)i];
    return PV_OK;
}

int pv_pool_blob_info(const void *blob, int64_t bytes, pv_pool_blob_desc *info) {
    g_last_error.clear();
    snap::Header h;
    if (!info) {
        g_last_error = "stream pool blob: no result structure";
        return PV_ERR_INVALID_ARG;
    }
    if (const char *why = snap::validate(blob, bytes, &h)) {
        g_last_error = std::string("stream pool blob: ") + why;
        return PV_ERR_INVALID_ARG;
    }
    *info = pv_pool_blob_desc{};
    info->version = (int32_t)h.version;
    info->arithmetic = h.arith;
    info->cfg = pv_config{h.sample_rate, h.channels, h.time_ratio, h.pitch_semitones, h.mode, h.coremode, h.fftsize, h.hopsize};
    info->time_ratio = h.time_ratio;
    info->pitch_semitones = h.pitch_semitones;
    info->slices = h.slices;
    info->pending_frames = h.pending;
    info->payload_bytes = snap::device_bytes(h);
    info->total_bytes = (int64_t)h.total_bytes;
    return PV_OK;
}

// ---------------------------------------------------------------- mixed batch
// Streams of different length, pitch and time ratio on the batch path (audiomod_pv.h "Mixed batch").  One Core holds
// the planes, state and rings of every stream (stream i owns rows [i*C, (i+1)*C), as a pool slot does); every stream
// has its own Derived, plan_batch() plan and ChainBuilder output, all built and uploaded once, at creation.  A launch
// group covers slices [g*Tc, (g+1)*Tc) of every stream that still has slices there; its PoolSlot / PoolParams / MbSlot
// tables are sorted by kernel variant like a mixed pool's feed.
} // extern "C"

struct pv_mbatch {
    // Everything on the device.  A redraw keeps it, growing what the new draw outgrows; only a draw whose largest
    // overlap-add advance exceeds what the Core's rings were sized for gets a new one (pv_mbatch_redraw).
    struct Dev {
        Core core;
        DevBuf<char> d_desc;       // the descriptor block (n: its capacity)
        DevBuf<float4> d_tabs;     // the sinc-table arena: one entry per distinct Speex num / den
        DevBuf<float> mix_stream;  // the overlap-add stream rings when the Core's own stream 0 does not resample
        struct Tab {
            uint32_t num, den;
        };
        std::vector<Tab> tabs;     // the arena's resident entries, in order
        size_t sinc4 = 0, tab_stride = 0, tab_cap = 0; // float4s of an entry's sinc part / of an entry; entries allocated
    };
    std::unique_ptr<Dev> dev;
    struct Span { // one per-sample array of one (stream, group) in the descriptor block (pv_mbatch_debug_descriptors)
        int64_t off, bytes;
        bool in_blob;
    };
    struct Stream {
        Derived d;
        BatchPlan plan;
        int64_t frames = 0, in_off = 0, out_off = 0;
        bool fast = false;
        int tab = -1, lds_floats = 0, tab_bytes = 0;
        std::vector<Span> wden, otab;
        float env_comp = 0.f; // the formant setting (pv_mbatch_set_formant): its PoolSlot::env_comp, 0 = off
        int voice = PV_VOICE_ROBOTIC; // the voice setting (pv_mbatch_set_voice)
    };
    std::vector<Stream> s; // (sized once per draw: the plans' builders keep references into it)
    int64_t in_floats = 0, out_floats = 0;
    struct Group {
        int64_t table_off = 0, params_off = 0, mb_off = 0;
        int nslots = 0, max_tn = 0;
        std::vector<VariantRun> vr;
        std::vector<int32_t> stream_of; // the stream of each table entry
        int fx_slots = 0;               // entries that run the formant stage
    };
    std::vector<Group> groups;
    int kernel_launches = 0; // kernels per run
    // The voice setting (pv_mbatch_set_voice): the phase table the whisper streams share, [slices][C][HP] from draw 0;
    // nothing exists before the first call with a whisper stream.
    DevBuf<float> d_voice;
    bool voice_on = false; // a stream has the whisper voice: the fused kernel's launches get the table
    bool tap_ran = false;    // pv_debug_mbatch_planes: a run since creation or the last redraw
    // what creation fixed (a redraw re-reads neither the arithmetic setting nor the environment)
    pv_config cfg{};
    int32_t block = 0, flush = 0;
    int device = 0, arith = PV_ARITH_EXACT, Tc = 0;
    bool has_runs_knob = false; // AUDIOMOD_PV_CHAIN_RUNS
    int runs_knob = 0;
    double plan_us = 0, host_us = 0, device_us = 0; // the last create or redraw (pv_mbatch_last_build_timing)
    // The PCM wire (pv_mbatch_run_pcm): nothing here exists before the first PCM run; buffers grow and never shrink.
    struct Pcm {
        DevBuf<float> stage;           // the run's float input, then (from out_base) its float output
        DevBuf<pv::MbPcmJob> jobs;     // n ingest jobs, then n egress jobs
        DevBuf<char> d_in, d_out;      // pv_mbatch_run_pcm_host's device PCM buffers
        std::vector<int32_t> bits;     // the depths the resident job table was built for (8 ... 32, never empty then)
        bool resident = false;         // false again after a redraw: the offsets have moved
        int64_t out_base = 0, in_bytes = 0, out_bytes = 0;
        int in_blocks = 0, out_blocks = 0;
    } pcm;
};

static const char *mb_scope(const pv_config &cfg) {
    switch (cfg.mode) {
    case PV_MODE_NORMAL_SHIFT: case PV_MODE_GENDER_CHANGE: case PV_MODE_FORMANT_PRESERVE: case PV_MODE_NORMAL_STRETCH:
    case PV_MODE_ROBOTIC: break;
    case PV_MODE_VOCODER_ROSENBERG: case PV_MODE_VOCODER_CHORD:
        return "mixed batch: the vocoder modes are not supported (their carrier planes are shared by all rows)";
    case PV_MODE_WHISPER: return "mixed batch: WHISPER is not supported (its phases come from one process-wide random stream)";
    case PV_MODE_CONSTANT: return "mixed batch: CONSTANT is not supported (its overrun flag is per stream)";
    case PV_MODE_FORMANT_CEPSTRAL: return "mixed batch: FORMANT_CEPSTRAL is not supported";
    default: return "mixed batch: unknown mode";
    }
    if (cfg.coremode < 0 || cfg.coremode > 2) return "mixed batch: coremodes 0-2 only";
    const int N = cfg.fftsize > 0 && cfg.fftsize <= 16384 ? next_pow2_i(cfg.fftsize) : 0;
    if (N < 512 || N > 4096)
        return "mixed batch: fftsize 512 ... 4096 only (the sizes of the fused synthesis + overlap-add kernel)";
    return nullptr;
}

// Everything that can be decided without a device: arguments, scope, every stream's constants and plan, the packing.
// arith: the pv_set_arithmetic setting the object was or is being created under
static int mb_plan(const pv_config *cfg, const pv_mbatch_stream *s, int32_t n, int32_t block, int32_t flush,
                   std::vector<pv_mbatch::Stream> &out, int arith) {
    g_last_error.clear();
    plan_reason_clear();
    if (!cfg || !s) {
        g_last_error = "mixed batch: null configuration or stream list";
        return PV_ERR_INVALID_ARG;
    }
    if (n < 1 || block < 1) {
        g_last_error = "mixed batch: nstreams and block must be at least 1";
        return PV_ERR_INVALID_ARG;
    }
    for (int32_t i = 0; i < n; ++i)
        if (s[i].frames < 1 || !std::isfinite(s[i].time_ratio) || !std::isfinite(s[i].pitch_semitones)) {
            g_last_error = "mixed batch: stream " + std::to_string(i) +
                           (s[i].frames < 1 ? ": frames must be at least 1" : ": pitch / time ratio is not a finite number");
            return PV_ERR_INVALID_ARG;
        }
    if (const char *why = mb_scope(*cfg)) {
        g_last_error = why;
        return PV_ERR_UNSUPPORTED;
    }
    if ((int64_t)n * cfg->channels > 65535) {
        g_last_error = "mixed batch: nstreams x channels above 65535 (the kernels put the slots on the grid's y / z)";
        return PV_ERR_UNSUPPORTED;
    }
    out.clear();
    out.resize((size_t)n);
    const int NR = arith == PV_ARITH_FAST ? (cfg->channels <= 2 ? 2 : cfg->channels <= 4 ? 4 : 8) : 4; // launch_mb_resample
    int64_t in_off = 0, out_off = 0;
    for (int32_t i = 0; i < n; ++i) {
        pv_mbatch::Stream &t = out[(size_t)i];
        pv_config ci = *cfg;
        ci.time_ratio = s[i].time_ratio;
        ci.pitch_semitones = s[i].pitch_semitones;
        int st = derive(ci, t.d);
        if (st == PV_OK) st = plan_batch(t.d, s[i].frames, block, flush != 0, t.plan);
        if (st != PV_OK) {
            const std::string why = g_last_error.empty() ? std::string(plan_reason()) : g_last_error;
            g_last_error = "mixed batch: stream " + std::to_string(i) + ": the engine refuses this configuration" +
                           (why.empty() ? std::string() : " (" + why + ")");
            return st;
        }
        const int nc = t.d.fft.nc;
        if (!(nc == 256 || nc == 512 || nc == 1024 || nc == 2048)) {
            g_last_error = "mixed batch: fftsize 512 ... 4096 only (the sizes of the fused synthesis + overlap-add kernel)";
            return PV_ERR_UNSUPPORTED;
        }
        if (t.d.resample) {
            t.lds_floats = pool_res_lds_floats(t.d);
            t.tab_bytes = res_tab_bytes(t.d);
            if ((size_t)t.tab_bytes + sizeof(float) * (size_t)t.lds_floats * NR > 160 * 1024 - 512) {
                g_last_error = "mixed batch: stream " + std::to_string(i) +
                               ": the resampling kernel's filter table and tile do not fit the LDS at this pitch";
                return PV_ERR_UNSUPPORTED;
            }
        }
        t.frames = s[i].frames;
        t.in_off = in_off;
        t.out_off = out_off;
        in_off += (int64_t)cfg->channels * t.frames;
        out_off += (int64_t)cfg->channels * t.plan.out_frames;
    }
    return PV_OK;
}

// kernels one launch group enqueues (mb_launch_group)
static int mb_group_kernels(const pv_mbatch::Group &g, int cm) {
    int k = 1 + (cm == 1 ? 2 : cm == 0 ? 1 : 0) + (g.fx_slots > 0 ? 1 : 0);
    for (size_t a = 0; a < g.vr.size();) {
        const size_t e = variant_group_end(g.vr, a);
        ++k;
        for (; a < e; ++a) k += g.vr[a].res && g.vr[a].max_tiles > 0 ? 1 : 0;
    }
    return k;
}

// the stages of one launch group (Core's argument builders with rows = C); launch = false: launch nothing,
// only ask the launchers whether this configuration fits them (pv_mbatch_create)
static int mb_launch_group(const pv_mbatch *b, const pv_mbatch::Group &g, const float *d_in, float *d_out, hipStream_t st,
                           bool launch = true) {
    const Core &c = b->dev->core;
    const char *desc = b->dev->d_desc.p;
    const Derived &d = c.d; // (only what every stream shares: sizes, mode, coremode)
    const int cm = phase_mode(d);
    const LaunchCheck lc{"mixed batch", "mixed batch: no ", nullptr, launch};
    int rc;
    const PoolLaunch pl{reinterpret_cast<const PoolSlot *>(desc + g.table_off), desc, d_out, g.nslots, g.max_tn, 0};
    const PoolParams *q = reinterpret_cast<const PoolParams *>(desc + g.params_off);
    const MbSlot *ms = reinterpret_cast<const MbSlot *>(desc + g.mb_off);
    if (launch) {
        AnalyzeArgs aa = c.analyze_args(c.C); // (its hop is stream 0's: the kernel takes each slot's from PoolParams)
        aa.ia.in = d_in; // (no ring: each slot's offset and length are in MbSlot)
        aa.ia.mask = ~0ull;
        if ((rc = lc.after(launch_mb_analyze(aa, pl, q, ms, st), "analysis")) != PV_OK) return rc;
    }
    if (cm == 1) {
        const MatchArgs ma = c.match_args(c.C);
        const SeqArgs qa = c.seq_args(c.C);
        if (launch) {
            launch_mb_match(ma, pl, q, st);
            if ((rc = lc.launched("match")) != PV_OK) return rc;
            if ((rc = lc.after(launch_mb_seq(qa, pl, q, st), "rotation chain")) != PV_OK) return rc;
        } else if (!pool_phase_supported(d.hs, c.PKP)) { // (the pool's bound: a deeper ring than launch_mb_seq's)
            return lc.refused("rotation chain");
        }
    } else if (cm == 0 && launch) {
        const PropArgs pa = c.prop_args(c.C);
        if ((rc = lc.after(launch_pmix_prop(pa, pl, q, st), "propagation")) != PV_OK) return rc;
    }
    if (launch && g.fx_slots > 0) // (the whole table: the slots with the setting off leave at their entry's 0)
        if ((rc = lc.after(launch_slot_cepstral(slot_cepstral_args(c), pl, PV_CENSUS_SET_MB, st), "formant")) != PV_OK) return rc;
    return launch_variant_groups(
        c, pl, g.vr, c.stream.p ? c.stream.p : b->dev->mix_stream.p, b->voice_on ? b->d_voice.p : nullptr,
        PoolCarrier(), lc, // (the carrier setting is the pools': audiomod_pv.h)
        [&](const SynthArgs &sa, const ChainArgs &ca, const PoolLaunch &sub, int first, int max_runs) {
            return launch_mb_synth_chain(sa, ca, sub, q + first, ms + first, max_runs, st, launch);
        },
        [&](const ResArgs &ra, const PoolLaunch &rs, int first) { return launch_mb_resample(ra, rs, q + first, st, launch); });
}

// What a create or redraw has prepared on the host and has yet to put on the device (mb_prepare -> mb_commit).
struct MbStage {
    DescBlob blob;              // the host-built part of the descriptor block
    int64_t dev_bytes = 0;      // the device-built part in front of it (redraw; 0: everything is in the blob)
    std::vector<MbWdenJob> wjobs;
    std::vector<MbOtabJob> ojobs;
    int wblocks = 0, oblocks = 0;
    int64_t wjobs_off = 0, ojobs_off = 0;
    // the sinc-table arena after this draw: its entries, geometry, the entries to upload, and a new buffer where the
    // resident one cannot take them
    std::vector<pv_mbatch::Dev::Tab> tabs;
    size_t sinc4 = 0, tab_stride = 0, tab_cap = 0;
    std::vector<std::pair<int, const Derived *>> tab_uploads;
    DevBuf<float4> new_tabs;
    bool replace_tabs = false, any_res = false;
};

// The sinc-table arena for the draw in b->s: streams with the same Speex num / den share an entry; entries already
// resident stay where they are and only new rate pairs are uploaded.  Where a new pair does not fit (no free entry, or a
// longer table than the entries were laid out for) the arena is laid out anew for this draw's pairs, with `slack`
// times as many entries.
static int mb_plan_tabs(pv_mbatch *b, bool fast_arith, int slack, MbStage &g) {
    const pv_mbatch::Dev &dv = *b->dev;
    struct Need {
        uint32_t num, den;
        const Derived *d;
    };
    std::vector<Need> need;
    size_t max_sinc4 = 0, max_tab4 = 0;
    for (pv_mbatch::Stream &t : b->s) {
        t.fast = Core::fast_capable_of(t.d, fast_arith);
        t.tab = -1;
        if (!t.d.resample) continue;
        g.any_res = true;
        bool seen = false;
        for (const Need &k : need) seen = seen || (k.num == t.d.res_num && k.den == t.d.res_den);
        if (seen) continue;
        need.push_back(Need{t.d.res_num, t.d.res_den, &t.d});
        max_sinc4 = std::max(max_sinc4, (t.d.sinc.size() + 3) / 4);
        if (t.d.interp) max_tab4 = std::max(max_tab4, (size_t)t.d.oversample * (t.d.filt_len + 1));
    }
    g.tabs = dv.tabs, g.sinc4 = dv.sinc4, g.tab_stride = dv.tab_stride, g.tab_cap = dv.tab_cap;
    bool fits = max_sinc4 <= dv.sinc4 && max_tab4 <= dv.tab_stride - dv.sinc4;
    if (fits)
        for (const Need &k : need) {
            bool resident = false;
            for (const pv_mbatch::Dev::Tab &r : g.tabs) resident = resident || (r.num == k.num && r.den == k.den);
            if (resident) continue;
            if (g.tabs.size() >= g.tab_cap) {
                fits = false;
                break;
            }
            g.tab_uploads.push_back({(int)g.tabs.size(), k.d});
            g.tabs.push_back(pv_mbatch::Dev::Tab{k.num, k.den});
        }
    if (!fits) {
        g.tabs.clear(), g.tab_uploads.clear();
        for (const Need &k : need) {
            g.tab_uploads.push_back({(int)g.tabs.size(), k.d});
            g.tabs.push_back(pv_mbatch::Dev::Tab{k.num, k.den});
        }
        g.sinc4 = std::max(max_sinc4, dv.sinc4);
        g.tab_stride = g.sinc4 + std::max(max_tab4, dv.tab_stride - dv.sinc4);
        g.tab_cap = need.size() * (size_t)slack;
        g.replace_tabs = true;
        const int st = g.new_tabs.alloc(g.tab_cap * g.tab_stride);
        if (st != PV_OK) return st;
    }
    for (pv_mbatch::Stream &t : b->s)
        for (size_t k = 0; k < g.tabs.size() && t.d.resample && t.tab < 0; ++k)
            if (g.tabs[k].num == t.d.res_num && g.tabs[k].den == t.d.res_den) t.tab = (int)k;
    return PV_OK;
}

// The descriptors of every (stream, group) -- phase increments, run lists, run offsets, denominators, resampling
// tiles -- then each group's tables, for the draw in b->s (mb_plan's) and the Core in b->dev.  Streams of equal
// parameters and length share their descriptors.  Host work only, apart from the allocation of a new table arena.
// on_device = false (pv_mbatch_create): everything goes into the blob.  on_device = true (pv_mbatch_redraw): the two
// per-sample arrays -- denominators and resampler output tables -- are only laid out, in a region in front of the
// blob, with one job each for the kernels that fill them.
static int mb_prepare(pv_mbatch *b, const pv_mbatch_stream *s, bool on_device, MbStage &stg) {
    const Core &c = b->dev->core;
    const int n = (int)b->s.size(), C = c.C, Tc = b->Tc;
    int st = mb_plan_tabs(b, c.fast_arith, on_device ? 2 : 1, stg);
    if (st != PV_OK) return st;
    const float4 *tab_base = stg.replace_tabs ? stg.new_tabs.p : b->dev->d_tabs.p;
    const int cm = phase_mode(c.d);
    int64_t maxT = 0;
    for (const pv_mbatch::Stream &t : b->s) maxT = std::max(maxT, (int64_t)t.plan.slices.size());
    const int G = (int)((maxT + Tc - 1) / Tc);
    std::vector<int> live((size_t)G, 0); // streams with slices in the group
    for (const pv_mbatch::Stream &t : b->s)
        for (int g = 0; (int64_t)g * Tc < (int64_t)t.plan.slices.size(); ++g) ++live[(size_t)g];
    DescBlob &blob = stg.blob;
    {
        size_t est = 1 << 20;
        for (const pv_mbatch::Stream &t : b->s)
            est += t.plan.slices.size() * (sizeof(ChainSlice) * 2 + 64) +
                   (on_device ? 0
                              : (size_t)t.plan.out_frames * 14 +
                                    (t.plan.slices.empty() ? 0 : (size_t)(t.plan.slices.back().P + t.d.N) * 5));
        blob.bytes.reserve(est);
    }
    auto reserve_dev = [&](size_t bytes) -> int64_t { // room in the device-built region (no host copy of it exists)
        const int64_t off = (stg.dev_bytes + 255) & ~(int64_t)255;
        stg.dev_bytes = off + (int64_t)bytes;
        return off;
    };
    struct Entry {
        PoolSlot ps;
        PoolParams q;
        MbSlot ms;
        int key;
        bool otab_in_blob;
    };
    std::vector<std::vector<Entry>> ent((size_t)G);
    std::vector<std::vector<Entry>> per_stream((size_t)n);
    std::vector<int32_t> pinc, ro, s_adv, s_wl;
    std::vector<int64_t> s_P;
    std::vector<float> wden, wden_hi;
    std::vector<ChainSlice> cs;
    std::vector<ResTile> res_tiles;
    std::vector<uint2> res_otab;
    for (int i = 0; i < n; ++i) {
        pv_mbatch::Stream &t = b->s[(size_t)i];
        const Derived &sd = t.d;
        const auto &sl = t.plan.slices;
        const int64_t T = (int64_t)sl.size();
        int twin = -1; // an earlier stream with the same constants and length: the same descriptors
        for (int j = 0; j < i && twin < 0; ++j)
            if (b->s[(size_t)j].frames == t.frames && s[j].time_ratio == s[i].time_ratio &&
                s[j].pitch_semitones == s[i].pitch_semitones)
                twin = j;
        std::vector<Entry> &mine = per_stream[(size_t)i];
        if (twin >= 0) {
            mine = per_stream[(size_t)twin];
            t.wden = b->s[(size_t)twin].wden, t.otab = b->s[(size_t)twin].otab;
        } else {
            ChainBuilder cb(sd, c.chain_AR, c.chain_smask);
            cb.count_only = on_device;
            // the kernel's 64-bit k * res_num must hold the stream's largest product (the host's is 128 bits wide)
            const bool otab_on_device =
                on_device && sd.resample &&
                ((unsigned __int128)(t.plan.out_frames + kTileOut) * sd.res_num >> 64) == 0;
            const size_t wj0 = stg.wjobs.size();
            int64_t p_off = 0, adv_off = 0;
            if (on_device) { // the per-slice records the denominator kernel reads, for the whole stream
                s_P.clear(), s_adv.clear(), s_wl.assign((size_t)T, 0);
                for (const SliceRec &r : sl) s_P.push_back(r.P), s_adv.push_back(r.adv);
                p_off = blob.put(s_P);
                adv_off = blob.put(s_adv);
            }
            for (int g = 0; (int64_t)g * Tc < T; ++g) {
                const int64_t t0 = (int64_t)g * Tc;
                const int Tn = (int)((T - t0) < Tc ? (T - t0) : Tc);
                const int64_t t1 = t0 + Tn;
                Entry e{};
                e.ps.t0 = t0;
                e.ps.s0 = (int32_t)(t0 % c.TR);
                e.ps.Tn = Tn;
                // the slot's own accumulator halves: launch g reads half g & 1 (nothing at the stream's start) and
                // writes the other
                e.ps.acc_sel = (g & 1) | (g == 0 ? 2 : 0);
                pinc.clear();
                for (int64_t k = t0; k < t1; ++k) pinc.push_back(sl[(size_t)k].phase_inc);
                e.ps.pinc_off = blob.put(pinc);
                wden.clear(), wden_hi.clear(), cs.clear(), ro.clear();
                const int64_t k0 = cb.begin_launch(sl[(size_t)t0]);
                for (int64_t k = t0; k < t1; ++k) cb.add(sl[(size_t)k], t.plan.out_frames, wden, wden_hi);
                if (on_device)
                    for (int k = 0; k < Tn; ++k)
                        s_wl[(size_t)(t0 + k)] = cb.launch_cs[(size_t)k].wden_off | (cb.launch_cs[(size_t)k].acc_pos & 3);
                // one workgroup per (row, run): split the slot's slices so that the group fills the chip, by
                // pv_batch_create's rule for the rows that are live in this group
                const int live_rows = live[(size_t)g] * C;
                int runs_wanted = (256 + live_rows - 1) / live_rows;
                if (live_rows > 256) { // a partly filled last round: best product of occupancy and useful share of a run
                    const double warm = (double)sd.N / (double)(sd.min_shift > 0 ? sd.min_shift : 1) + 1.0;
                    double best = 0.0;
                    for (int r = 1; r <= 8; ++r) {
                        const double wgs = (double)live_rows * r / 256.0, len = (double)Tn / r;
                        const double eff = wgs / std::ceil(wgs) * (r == 1 ? 1.0 : len / (len + warm));
                        if (eff > best + 1e-9) best = eff, runs_wanted = r;
                    }
                }
                if (b->has_runs_knob) runs_wanted = b->runs_knob;
                e.ms.runs = cb.end_launch(runs_wanted > 32 ? 32 : runs_wanted, cs, ro);
                while (ro.size() & 3) ro.push_back(0);
                e.ps.cs_off = blob.put(cs);
                e.ps.ro_off = blob.put(ro);
                if (on_device) { // (every slice's entries are whole quads: no padding before the four trailing ones)
                    MbWdenJob jb{};
                    jb.total = (int32_t)(cb.wden_count + 4);
                    jb.dst_off = e.ps.wden_off = reserve_dev((size_t)jb.total * sizeof(float));
                    jb.p_off = p_off, jb.adv_off = adv_off;
                    jb.t0 = (int32_t)t0, jb.Tn = Tn;
                    jb.first_block = stg.wblocks;
                    jb.N = sd.N, jb.fast = t.fast ? 1 : 0;
                    jb.win_gain = sd.win_gain;
                    stg.wblocks += mb_build_wden_blocks(jb.total);
                    stg.wjobs.push_back(jb);
                    t.wden.push_back(pv_mbatch::Span{jb.dst_off, (int64_t)jb.total * (int64_t)sizeof(float), false});
                } else {
                    finish_wden(wden, t.fast);
                    e.ps.wden_off = blob.put(wden);
                    t.wden.push_back(pv_mbatch::Span{e.ps.wden_off, (int64_t)(wden.size() * sizeof(float)), true});
                }
                int64_t ka = sl[(size_t)t0].K0, kb = sl[(size_t)(t1 - 1)].K0 + sl[(size_t)(t1 - 1)].cnt;
                if (ka > t.plan.out_frames) ka = t.plan.out_frames;
                if (kb > t.plan.out_frames) kb = t.plan.out_frames;
                res_tiles.clear(), res_otab.clear();
                if (sd.resample && kb > ka) build_res_tiles_of(sd, ka, kb, res_tiles, res_otab, otab_on_device);
                e.ps.res_ntiles = (int32_t)res_tiles.size();
                e.ps.res_off = blob.put(res_tiles);
                e.otab_in_blob = !(otab_on_device && !res_tiles.empty());
                if (e.otab_in_blob) {
                    e.ps.otab_off = blob.put(res_otab);
                    t.otab.push_back(pv_mbatch::Span{e.ps.otab_off, (int64_t)(res_otab.size() * sizeof(uint2)), true});
                } else {
                    MbOtabJob jb{};
                    jb.ntiles = (int32_t)res_tiles.size();
                    const size_t bytes = res_tiles.size() * (size_t)kTileOut * sizeof(uint2);
                    jb.dst_off = e.ps.otab_off = reserve_dev(bytes);
                    jb.ka = ka, jb.kb = kb;
                    jb.res_num = sd.res_num, jb.res_den = sd.res_den;
                    jb.filt_len = sd.filt_len, jb.oversample = sd.oversample, jb.interp = sd.interp ? 1 : 0;
                    jb.first_block = stg.oblocks;
                    stg.oblocks += mb_build_otab_blocks(jb.ntiles);
                    stg.ojobs.push_back(jb);
                    t.otab.push_back(pv_mbatch::Span{jb.dst_off, (int64_t)bytes, false});
                }
                e.ps.out_off = k0; // (+ the stream's own offset, below)
                e.ps.out_stride_row = t.plan.out_frames;
                e.ps.k_base = k0;
                e.ps.wh_off = -1; // (pv_mbatch_set_voice patches it)
                e.ps.car_off = -1;
                e.q = slot_params(sd, t.tab_bytes, t.lds_floats,
                                  sd.resample ? tab_base + (size_t)t.tab * stg.tab_stride : nullptr, stg.sinc4);
                e.key = variant_key(sd, t.fast);
                mine.push_back(e);
            }
            if (on_device) {
                const int64_t wl_off = blob.put(s_wl);
                for (size_t k = wj0; k < stg.wjobs.size(); ++k) stg.wjobs[k].woff_off = wl_off;
            }
        }
        for (size_t g = 0; g < mine.size(); ++g) {
            Entry e = mine[g];
            e.ps.row0 = i * C;
            e.ps.out_off += t.out_off;
            e.ms.in_off = t.in_off;
            e.ms.frames = t.frames;
            ent[g].push_back(e);
        }
    }
    // the blob follows the device-built region: what points into it moves by the region's size
    stg.dev_bytes = (stg.dev_bytes + 255) & ~(int64_t)255;
    const int64_t shift = stg.dev_bytes;
    for (pv_mbatch::Stream &t : b->s) {
        for (pv_mbatch::Span &sp : t.wden) sp.off += sp.in_blob ? shift : 0;
        for (pv_mbatch::Span &sp : t.otab) sp.off += sp.in_blob ? shift : 0;
    }
    for (MbWdenJob &jb : stg.wjobs) jb.p_off += shift, jb.adv_off += shift, jb.woff_off += shift;
    b->groups.assign((size_t)G, pv_mbatch::Group());
    b->kernel_launches = 0;
    std::vector<PoolSlot> table;
    std::vector<PoolParams> params;
    std::vector<MbSlot> mbs;
    for (int g = 0; g < G; ++g) {
        std::vector<Entry> &ev = ent[(size_t)g];
        // slots of one variant contiguous (stable: stream order otherwise)
        std::stable_sort(ev.begin(), ev.end(), [](const Entry &x, const Entry &y) { return x.key < y.key; });
        pv_mbatch::Group &gr = b->groups[(size_t)g];
        table.clear(), params.clear(), mbs.clear();
        for (size_t k = 0; k < ev.size(); ++k) {
            Entry &e = ev[k];
            e.ps.pinc_off += shift, e.ps.cs_off += shift, e.ps.ro_off += shift, e.ps.res_off += shift;
            if (!on_device) e.ps.wden_off += shift;
            if (e.otab_in_blob) e.ps.otab_off += shift;
            variant_runs_add(gr.vr, (int)k, e.key, e.ps.res_ntiles, e.q.lds_floats, e.q.tab_bytes, e.ms.runs);
            gr.max_tn = std::max(gr.max_tn, (int)e.ps.Tn);
            table.push_back(e.ps), params.push_back(e.q), mbs.push_back(e.ms);
            gr.stream_of.push_back(e.ps.row0 / C);
        }
        gr.nslots = (int)ev.size();
        gr.table_off = shift + blob.put(table);
        gr.params_off = shift + blob.put(params);
        gr.mb_off = shift + blob.put(mbs);
        b->kernel_launches += mb_group_kernels(gr, cm);
    }
    stg.wjobs_off = shift + blob.put(stg.wjobs);
    stg.ojobs_off = shift + blob.put(stg.ojobs);
    return PV_OK;
}

// every variant present against its launcher's limits (launches nothing)
static int mb_check_groups(const pv_mbatch *b) {
    for (const pv_mbatch::Group &gr : b->groups) {
        const int st = mb_launch_group(b, gr, nullptr, nullptr, nullptr, false);
        if (st != PV_OK) return st;
    }
    return PV_OK;
}

// Puts what mb_prepare staged on the device: new table-arena entries, the blob, and -- a redraw -- the two build
// kernels over the region in front of it.  Everything that can fail for lack of memory comes first; nothing resident
// is written before it.  grow: allocate an eighth more than needed (a redraw's next draw is about as long).
static int mb_commit(pv_mbatch *b, MbStage &stg, bool grow) {
    pv_mbatch::Dev &dv = *b->dev;
    const Core &c = dv.core;
    int st;
    const size_t need = (size_t)stg.dev_bytes + stg.blob.bytes.size();
    if (need > dv.d_desc.n || !dv.d_desc.p) {
        DevBuf<char> fresh;
        if ((st = fresh.alloc(need + (grow ? need / 8 : 0))) != PV_OK) return st;
        dv.d_desc.swap(fresh);
    }
#ifdef PV_POISON // an entry the builders forget to write shows as NaN / -1, not as the draw before's value
    else HIPC(hipMemset(dv.d_desc.p, 0xFF, dv.d_desc.n));
#endif
    if (stg.any_res && !c.stream.p && !dv.mix_stream.p)
        if ((st = dv.mix_stream.alloc((size_t)c.rows * ((size_t)c.chain_smask + 1))) != PV_OK) return st;
    if (stg.replace_tabs) dv.d_tabs.swap(stg.new_tabs);
    dv.tabs = stg.tabs, dv.sinc4 = stg.sinc4, dv.tab_stride = stg.tab_stride, dv.tab_cap = stg.tab_cap;
    std::vector<float4> img;
    for (const auto &up : stg.tab_uploads) {
        slot_tab_image(*up.second, dv.tab_stride, dv.sinc4, img);
        HIPC(hipMemcpy(dv.d_tabs.p + (size_t)up.first * dv.tab_stride, img.data(), img.size() * sizeof(float4),
                       hipMemcpyHostToDevice));
    }
    if (!stg.blob.bytes.empty())
        HIPC(hipMemcpy(dv.d_desc.p + stg.dev_bytes, stg.blob.bytes.data(), stg.blob.bytes.size(), hipMemcpyHostToDevice));
    launch_mb_build_wden(reinterpret_cast<const MbWdenJob *>(dv.d_desc.p + stg.wjobs_off), (int)stg.wjobs.size(), stg.wblocks,
                         dv.d_desc.p, c.window.p, nullptr);
    launch_mb_build_otab(reinterpret_cast<const MbOtabJob *>(dv.d_desc.p + stg.ojobs_off), (int)stg.ojobs.size(), stg.oblocks,
                         dv.d_desc.p, nullptr);
    HIPC(hipGetLastError());
    return PV_OK;
}

static int mb_chunk_slices(int rows) {
    // slices per launch and slot: as pv_batch_create sizes its chunks (the fused path's wide ones: every stream here
    // takes the fused path), AUDIOMOD_PV_CHUNK_SLICES included
    int Tc = 131072 / rows;
    if (Tc < 16) Tc = 16;
    if (Tc > 512) Tc = 512;
    if (const char *env = getenv("AUDIOMOD_PV_CHUNK_SLICES")) {
        const int v = atoi(env);
        if (v >= 4 && v <= 1024) Tc = v;
    }
    return Tc;
}

static int mb_max_adv(const std::vector<pv_mbatch::Stream> &v) {
    int mx = 1; // the overlap-add rings are sized from the advances the plans really contain
    for (const pv_mbatch::Stream &t : v)
        for (const SliceRec &r : t.plan.slices) mx = r.adv > mx ? r.adv : mx;
    return mx;
}

// a Core for b's configuration with rings for advances up to max_adv (its own constants: those of stream s0; only what
// every stream shares is read from them)
static int mb_init_core(const pv_mbatch *b, pv_mbatch::Dev &dv, const pv_mbatch_stream &s0, int max_adv) {
    Core &c = dv.core;
    c.chain_required = true;
    c.fast_arith = b->arith == PV_ARITH_FAST;
    c.chain_max_adv = max_adv;
    pv_config c0 = b->cfg;
    c0.time_ratio = s0.time_ratio;
    c0.pitch_semitones = s0.pitch_semitones;
    const int st = c.init(c0, b->device, (int)b->s.size(), b->Tc);
    if (st != PV_OK) return st;
    // (chain_waves: init takes sixteen waves for a plain stream 0 and twelve otherwise, eight at fft 4096; the per-slot
    // fused kernels are compiled for at most twelve and their launcher clamps to that, so every variant of the corpus
    // runs with the same wave count whichever stream comes first)
    if (!c.use_chain || !c.wave_fft()) {
        g_last_error = "mixed batch: needs the fused synthesis + overlap-add path (AUDIOMOD_PV_FUSED=0 turns it off)";
        return PV_ERR_UNSUPPORTED;
    }
    return PV_OK;
}

static double mb_us(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
    return std::chrono::duration<double, std::micro>(b - a).count();
}

extern "C" {

int pv_mbatch_layout(const pv_config *cfg, const pv_mbatch_stream *s, int32_t nstreams, int32_t block, int32_t flush,
                     int64_t *out_frames, int64_t *slices, int64_t *in_off, int64_t *out_off, int64_t *in_floats,
                     int64_t *out_floats) {
    std::vector<pv_mbatch::Stream> v;
    const int st = mb_plan(cfg, s, nstreams, block, flush, v, g_arith);
    if (st != PV_OK) return st;
    for (size_t i = 0; i < v.size(); ++i) {
        if (out_frames) out_frames[i] = v[i].plan.out_frames;
        if (slices) slices[i] = (int64_t)v[i].plan.slices.size();
        if (in_off) in_off[i] = v[i].in_off;
        if (out_off) out_off[i] = v[i].out_off;
    }
    if (in_floats) *in_floats = v.back().in_off + (int64_t)cfg->channels * v.back().frames;
    if (out_floats) *out_floats = v.back().out_off + (int64_t)cfg->channels * v.back().plan.out_frames;
    return PV_OK;
}

int pv_mbatch_create(const pv_config *cfg, const pv_mbatch_stream *s, int32_t nstreams, int32_t block, int32_t flush,
                     int device, pv_mbatch **out) {
    if (out) *out = nullptr;
    const auto t_begin = std::chrono::steady_clock::now();
    std::unique_ptr<pv_mbatch> b(new pv_mbatch());
    int st = mb_plan(cfg, s, nstreams, block, flush, b->s, g_arith);
    if (st != PV_OK) return st;
    const auto t_planned = std::chrono::steady_clock::now();
    if (!out) {
        g_last_error = "mixed batch: null handle pointer";
        return PV_ERR_INVALID_ARG;
    }
    const int C = cfg->channels;
    b->in_floats = b->s.back().in_off + (int64_t)C * b->s.back().frames;
    b->out_floats = b->s.back().out_off + (int64_t)C * b->s.back().plan.out_frames;
    b->cfg = *cfg, b->block = block, b->flush = flush, b->device = device, b->arith = g_arith;
    b->Tc = mb_chunk_slices(nstreams * C);
    if (const char *runs_env = getenv("AUDIOMOD_PV_CHAIN_RUNS")) // tuning knob, as pv_batch_create reads it
        b->has_runs_knob = true, b->runs_knob = atoi(runs_env);
    b->dev.reset(new pv_mbatch::Dev());
    if ((st = mb_init_core(b.get(), *b->dev, s[0], mb_max_adv(b->s))) != PV_OK) return st;
    MbStage stg;
    if ((st = mb_prepare(b.get(), s, false, stg)) != PV_OK) return st;
    if ((st = mb_commit(b.get(), stg, false)) != PV_OK) return st;
    if ((st = mb_check_groups(b.get())) != PV_OK) return st;
    b->plan_us = mb_us(t_begin, t_planned);
    b->host_us = mb_us(t_planned, std::chrono::steady_clock::now());
    b->device_us = 0;
    *out = b.release();
    return PV_OK;
}

// pv_mbatch_redraw: audiomod_pv.h.  Order: every check first (mb_plan on a staging object, the launchers' limits
// against the Core the draw will run on), then the device is synchronised -- an earlier run may still read the
// descriptors -- and only then anything resident is written.
int pv_mbatch_redraw(pv_mbatch *b, const pv_mbatch_stream *s) {
    g_last_error.clear();
    plan_reason_clear();
    if (!b || !s) {
        g_last_error = "mixed batch: null object or stream list";
        return PV_ERR_INVALID_ARG;
    }
    const auto t_begin = std::chrono::steady_clock::now();
    std::unique_ptr<pv_mbatch> nb(new pv_mbatch());
    const int n = (int)b->s.size(), C = b->cfg.channels;
    int st = mb_plan(&b->cfg, s, n, b->block, b->flush, nb->s, b->arith);
    if (st != PV_OK) return st;
    const auto t_planned = std::chrono::steady_clock::now();
    nb->in_floats = nb->s.back().in_off + (int64_t)C * nb->s.back().frames;
    nb->out_floats = nb->s.back().out_off + (int64_t)C * nb->s.back().plan.out_frames;
    nb->cfg = b->cfg, nb->block = b->block, nb->flush = b->flush, nb->device = b->device, nb->arith = b->arith;
    nb->Tc = b->Tc, nb->has_runs_knob = b->has_runs_knob, nb->runs_knob = b->runs_knob;
    HIPC(hipSetDevice(b->device));
    // The Core: kept unless the draw's largest advance exceeds what its rings were sized for; then a new one, sized as
    // pv_mbatch_create would size it, beside the old one until the checks have passed (the slow path: Core::init again).
    const int mx = mb_max_adv(nb->s);
    const bool rebuild = mx > b->dev->core.chain_max_adv;
    if (rebuild) {
        nb->dev.reset(new pv_mbatch::Dev());
        if ((st = mb_init_core(nb.get(), *nb->dev, s[0], mx)) != PV_OK) return st;
    } else {
        nb->dev = std::move(b->dev); // (on loan while the draw is prepared and checked)
    }
    auto refuse = [&](int status) {
        if (!rebuild) b->dev = std::move(nb->dev);
        return status;
    };
    MbStage stg;
    if ((st = mb_prepare(nb.get(), s, true, stg)) != PV_OK) return refuse(st);
    if ((st = mb_check_groups(nb.get())) != PV_OK) return refuse(st);
    {
        const hipError_t e = hipDeviceSynchronize();
        if (e != hipSuccess) return refuse(hip_fail(e, "hipDeviceSynchronize", __LINE__));
    }
    if ((st = mb_commit(nb.get(), stg, true)) != PV_OK) return refuse(st);
    const auto t_host = std::chrono::steady_clock::now();
    {
        const hipError_t e = hipDeviceSynchronize(); // the build kernels: a run may follow on any stream
        if (e != hipSuccess) return refuse(hip_fail(e, "mixed batch descriptor build", __LINE__));
    }
    const auto t_done = std::chrono::steady_clock::now();
    b->dev = std::move(nb->dev);
    b->s = std::move(nb->s);
    b->groups = std::move(nb->groups);
    b->in_floats = nb->in_floats, b->out_floats = nb->out_floats, b->kernel_launches = nb->kernel_launches;
    b->pcm.resident = false; // (the next PCM run builds its job table for the new offsets)
    b->voice_on = false;     // (every stream of the new draw is robotic: its tables say -1)
    b->tap_ran = false;      // (the planes still hold the previous draw's slices)
    b->plan_us = mb_us(t_begin, t_planned), b->host_us = mb_us(t_planned, t_host), b->device_us = mb_us(t_host, t_done);
    return PV_OK;
}

int pv_mbatch_last_build_timing(const pv_mbatch *b, double *plan_us, double *host_us, double *device_us) {
    if (!b) return PV_ERR_INVALID_ARG;
    if (plan_us) *plan_us = b->plan_us;
    if (host_us) *host_us = b->host_us;
    if (device_us) *device_us = b->device_us;
    return PV_OK;
}

int64_t pv_mbatch_debug_descriptors(const pv_mbatch *b, int32_t stream, int which, void *out, int64_t max_bytes) {
    g_last_error.clear();
    if (!b || stream < 0 || (size_t)stream >= b->s.size() || (which != PV_MB_DESC_WDEN && which != PV_MB_DESC_OTAB) ||
        max_bytes < 0 || (!out && max_bytes > 0))
        return -(int64_t)PV_ERR_INVALID_ARG;
    const std::vector<pv_mbatch::Span> &v = which == PV_MB_DESC_WDEN ? b->s[(size_t)stream].wden : b->s[(size_t)stream].otab;
    int64_t total = 0;
    for (const pv_mbatch::Span &sp : v) total += sp.bytes;
    if (hipSetDevice(b->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -(int64_t)PV_ERR_HIP;
    int64_t done = 0;
    for (const pv_mbatch::Span &sp : v) {
        const int64_t take = std::min(sp.bytes, max_bytes - done);
        if (take <= 0) break;
        if (hipMemcpy((char *)out + done, b->dev->d_desc.p + sp.off, (size_t)take, hipMemcpyDeviceToHost) != hipSuccess)
            return -(int64_t)PV_ERR_HIP;
        done += take;
    }
    return total;
}

void pv_mbatch_destroy(pv_mbatch *b) { delete b; }
int32_t pv_mbatch_nstreams(const pv_mbatch *b) { return b ? (int32_t)b->s.size() : -1; }
static bool mb_index_ok(const pv_mbatch *b, int32_t i) { return b && i >= 0 && (size_t)i < b->s.size(); }
int64_t pv_mbatch_out_frames(const pv_mbatch *b, int32_t i) { return mb_index_ok(b, i) ? b->s[(size_t)i].plan.out_frames : -1; }
int64_t pv_mbatch_in_offset(const pv_mbatch *b, int32_t i) { return mb_index_ok(b, i) ? b->s[(size_t)i].in_off : -1; }
int64_t pv_mbatch_out_offset(const pv_mbatch *b, int32_t i) { return mb_index_ok(b, i) ? b->s[(size_t)i].out_off : -1; }
int64_t pv_mbatch_in_floats(const pv_mbatch *b) { return b ? b->in_floats : -1; }
int64_t pv_mbatch_out_floats(const pv_mbatch *b) { return b ? b->out_floats : -1; }
int32_t pv_mbatch_launches(const pv_mbatch *b) { return b ? (int32_t)b->groups.size() : -1; }
int32_t pv_mbatch_kernel_launches(const pv_mbatch *b) { return b ? (int32_t)b->kernel_launches : -1; }

int pv_mbatch_get_info(const pv_mbatch *b, int32_t i, pv_info *info) {
    if (!mb_index_ok(b, i) || !info) return PV_ERR_INVALID_ARG;
    fill_info(b->s[(size_t)i].d, (int64_t)b->s[(size_t)i].plan.slices.size(), info);
    return PV_OK;
}

int pv_mbatch_run(pv_mbatch *b, const float *d_in, float *d_out, void *hip_stream) {
    g_last_error.clear();
    plan_reason_clear();
    if (!b || !d_in || (!d_out && b->out_floats > 0)) return PV_ERR_INVALID_ARG; // an empty output needs no buffer
    Core &c = b->dev->core;
    hipStream_t st = (hipStream_t)hip_stream;
    HIPC(hipSetDevice(c.device));
    int rc = c.reset_state(st); // every run starts every stream afresh (the accumulator halves restart with the plan's)
    if (rc != PV_OK) return rc;
    for (const pv_mbatch::Group &g : b->groups)
        if ((rc = mb_launch_group(b, g, d_in, d_out, st)) != PV_OK) return rc;
    HIPC(hipGetLastError());
    b->tap_ran = true;
    return PV_OK;
}

// pv_mbatch_set_formant: audiomod_pv.h.  The slot tables are resident, so the setting is written into them: every check
// first, then the device is synchronised -- an earlier run may still read the tables, as in pv_mbatch_redraw -- and the
// env_comp field of every group's entries is patched, one strided copy per group.
int pv_mbatch_set_formant(pv_mbatch *b, const float *formant_semitones) {
    g_last_error.clear();
    plan_reason_clear();
    if (!b) return PV_ERR_INVALID_ARG;
    int st = formant_scope_check(b->cfg);
    if (st != PV_OK) return st;
    const size_t n = b->s.size();
    std::vector<float> env(n, 0.f);
    for (size_t i = 0; i < n && formant_semitones; ++i) {
        const float v = formant_semitones[i];
        if (std::isnan(v)) continue; // off
        if ((st = formant_value_check(v)) != PV_OK) {
            g_last_error = "mixed batch: stream " + std::to_string(i) + ": " + g_last_error;
            return st;
        }
        const float e = formant_env_comp_of(b->s[i].d.pitch_scale, v);
        env[i] = e != 1.0f ? e : 0.f; // (as mode FORMANT_CEPSTRAL skips the stage at pitch scale 1)
    }
    HIPC(hipSetDevice(b->device));
    HIPC(hipDeviceSynchronize());
    const int cm = phase_mode(b->dev->core.d);
    std::vector<float> col;
    int launches = 0;
    for (pv_mbatch::Group &g : b->groups) {
        col.clear();
        g.fx_slots = 0;
        for (const int32_t i : g.stream_of) {
            col.push_back(env[(size_t)i]);
            g.fx_slots += env[(size_t)i] != 0.f ? 1 : 0;
        }
        if (!col.empty())
            HIPC(hipMemcpy2D(b->dev->d_desc.p + g.table_off + offsetof(PoolSlot, env_comp), sizeof(PoolSlot), col.data(),
                             sizeof(float), sizeof(float), col.size(), hipMemcpyHostToDevice));
        launches += mb_group_kernels(g, cm);
    }
    for (size_t i = 0; i < n; ++i) b->s[i].env_comp = env[i];
    b->kernel_launches = launches;
    return PV_OK;
}

// pv_mbatch_set_voice: audiomod_pv.h.  Every run starts every stream at draw 0, so the whisper streams share ONE table
// of phases, [slices of the longest whisper stream][C][HP], drawn here by one generator launch -- a wave per 64 rows,
// each from the state the host's jump-ahead gives it; a run launches nothing more than before.  The resident slot tables get each entry's offset into it (its first slice
// times C * HP, or -1), one strided copy per group, behind a device synchronisation as in pv_mbatch_set_formant.
int pv_mbatch_set_voice(pv_mbatch *b, const int32_t *voice) {
    g_last_error.clear();
    plan_reason_clear();
    if (!b) return PV_ERR_INVALID_ARG;
    int st = voice_scope_check(b->cfg);
    if (st != PV_OK) return st;
    const size_t n = b->s.size();
    int64_t slices = 0;
    for (size_t i = 0; i < n && voice; ++i) {
        if ((st = voice_value_check(voice[i])) != PV_OK) {
            g_last_error = "mixed batch: stream " + std::to_string(i) + ": " + g_last_error;
            return st;
        }
        if (voice[i] == PV_VOICE_WHISPER) slices = std::max(slices, (int64_t)b->s[i].plan.slices.size());
    }
    const Core &c = b->dev->core;
    const int64_t row = (int64_t)c.C * c.HP;
    HIPC(hipSetDevice(b->device));
    HIPC(hipDeviceSynchronize());
    if (slices > 0) {
        // The table's rows in chunks of kVoiceChunkRows, one wave each: chunk k starts k * D draws on, from a state the
        // host makes by jump-ahead (pv_whisper.h) -- chunk by chunk, each from the one before.
        constexpr int64_t kVoiceChunkRows = 64;
        const int32_t per = c.d.hs + 1;
        const int64_t rows = slices * c.C, nchunks = (rows + kVoiceChunkRows - 1) / kVoiceChunkRows;
        std::vector<uint32_t> states((size_t)nchunks * kWhisperStatePitch, 0);
        std::vector<WhisperJob> jobs((size_t)nchunks);
        uint32_t poly[31];
        whisper_jump_poly((uint64_t)kVoiceChunkRows * per, poly);
        memcpy(states.data(), whisper_fresh_state().data(), (size_t)kWhisperHist * sizeof(uint32_t));
        for (int64_t k = 0; k < nchunks; ++k) {
            if (k > 0) whisper_state_jump(&states[(size_t)(k - 1) * kWhisperStatePitch], poly, &states[(size_t)k * kWhisperStatePitch]);
            WhisperJob &wj = jobs[(size_t)k];
            wj.src_off = k * kWhisperStatePitch, wj.dst_off = -1; // (the next run starts afresh: no state is kept)
            wj.out_off = k * kVoiceChunkRows * c.HP;
            wj.count = std::min(kVoiceChunkRows, rows - k * kVoiceChunkRows) * per;
            wj.per = per, wj.pitch = c.HP;
        }
        if ((size_t)(slices * row) > b->d_voice.n && (st = b->d_voice.alloc((size_t)(slices * row))) != PV_OK) return st;
        DevBuf<uint32_t> d_states;
        DevBuf<WhisperJob> d_jobs;
        if ((st = d_states.upload(states)) != PV_OK || (st = d_jobs.upload(jobs)) != PV_OK) return st;
        launch_whisper(d_states.p, b->d_voice.p, d_jobs.p, (int)nchunks, PV_CENSUS_SET_MB, c.d.fft.nc, nullptr);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "voice generator launch", __LINE__);
        HIPC(hipDeviceSynchronize()); // (a run may follow on any stream; the two buffers above go)
    }
    std::vector<int64_t> col;
    for (pv_mbatch::Group &g : b->groups) {
        col.clear();
        const int64_t gi = &g - b->groups.data();
        for (const int32_t i : g.stream_of)
            col.push_back(voice && voice[(size_t)i] == PV_VOICE_WHISPER ? gi * b->Tc * row : (int64_t)-1);
        if (!col.empty())
            HIPC(hipMemcpy2D(b->dev->d_desc.p + g.table_off + offsetof(PoolSlot, wh_off), sizeof(PoolSlot), col.data(),
                             sizeof(int64_t), sizeof(int64_t), col.size(), hipMemcpyHostToDevice));
    }
    for (size_t i = 0; i < n; ++i) b->s[i].voice = voice ? voice[i] : PV_VOICE_ROBOTIC;
    b->voice_on = slices > 0;
    return PV_OK;
}

} // extern "C"

// ---------------------------------------------------------------- mixed batch, PCM wire (audiomod_pv.h)
static bool mb_pcm_depth_ok(int32_t bits) { return bits == 8 || bits == 16 || bits == 24 || bits == 32; }

// the arguments every PCM entry checks, before any device call
static int mb_pcm_check(const pv_mbatch *b, const int32_t *in_bits) {
    g_last_error.clear();
    if (!b) {
        g_last_error = "mixed batch PCM: null object";
        return PV_ERR_INVALID_ARG;
    }
    for (size_t i = 0; in_bits && i < b->s.size(); ++i)
        if (!mb_pcm_depth_ok(in_bits[i])) {
            g_last_error = "mixed batch PCM: stream " + std::to_string(i) + ": " + std::to_string(in_bits[i]) +
                           " bits per sample (8, 16, 24 or 32)";
            return PV_ERR_INVALID_ARG;
        }
    return PV_OK;
}

struct MbPcmLayout {
    std::vector<int64_t> in_off, out_off;
    int64_t in_bytes = 0, out_bytes = 0;
};
static MbPcmLayout mb_pcm_layout(const pv_mbatch *b, const int32_t *in_bits) {
    MbPcmLayout l;
    const int64_t C = b->cfg.channels;
    for (size_t i = 0; i < b->s.size(); ++i) {
        l.in_off.push_back(l.in_bytes);
        l.out_off.push_back(l.out_bytes);
        l.in_bytes += (b->s[i].frames * C * ((in_bits ? in_bits[i] : 16) / 8) + 15) & ~(int64_t)15;
        l.out_bytes += (b->s[i].plan.out_frames * C * 2 + 15) & ~(int64_t)15;
    }
    return l;
}

// The staging buffers and the job table for `in_bits`.  Nothing to do when the table for these depths is resident;
// otherwise the device is synchronised first (an earlier run may still use what is replaced) and again afterwards
// (the fills and the upload are on the default stream, which nothing orders against a non-blocking one).
static int mb_pcm_prepare(pv_mbatch *b, const int32_t *in_bits) {
    pv_mbatch::Pcm &p = b->pcm;
    const size_t n = b->s.size();
    std::vector<int32_t> bits(n, 16);
    if (in_bits) bits.assign(in_bits, in_bits + n);
    if (p.resident && bits == p.bits) return PV_OK;
    const int C = b->cfg.channels;
    const MbPcmLayout l = mb_pcm_layout(b, bits.data());
    std::vector<MbPcmJob> jobs(2 * n);
    const int64_t out_base = (b->in_floats + 63) & ~(int64_t)63;
    int64_t blocks[2] = {0, 0};
    for (size_t i = 0; i < n; ++i) {
        const pv_mbatch::Stream &t = b->s[i];
        jobs[i] = MbPcmJob{l.in_off[i], t.in_off, t.frames, C, bits[i] / 8, (int32_t)blocks[0], 0};
        // (planar offsets count from the pointer the launch is given: the stage's input part, its output part)
        jobs[n + i] = MbPcmJob{l.out_off[i], t.out_off, t.plan.out_frames, C, 2, (int32_t)blocks[1], 0};
        blocks[0] += mb_pcm_blocks(t.frames, C);
        blocks[1] += mb_pcm_blocks(t.plan.out_frames, C);
        if (blocks[0] > 0x7fffffff || blocks[1] > 0x7fffffff) {
            g_last_error = "mixed batch PCM: more conversion tiles than one launch's grid holds";
            return PV_ERR_UNSUPPORTED;
        }
    }
    HIPC(hipDeviceSynchronize());
    int st;
    const size_t need = (size_t)(out_base + b->out_floats);
    if ((need > p.stage.n || !p.stage.p) && (st = p.stage.alloc(need)) != PV_OK) return st;
    if ((jobs.size() > p.jobs.n || !p.jobs.p) && (st = p.jobs.alloc(jobs.size())) != PV_OK) return st;
    p.resident = false;
    HIPC(hipMemcpy(p.jobs.p, jobs.data(), jobs.size() * sizeof(MbPcmJob), hipMemcpyHostToDevice));
    HIPC(hipDeviceSynchronize());
    p.bits = bits, p.out_base = out_base, p.in_bytes = l.in_bytes, p.out_bytes = l.out_bytes;
    p.in_blocks = (int)blocks[0], p.out_blocks = (int)blocks[1];
    p.resident = true;
    return PV_OK;
}

extern "C" {

int pv_mbatch_pcm_layout(const pv_mbatch *b, const int32_t *in_bits, int64_t *in_byte_off, int64_t *out_byte_off,
                         int64_t *in_bytes, int64_t *out_bytes) {
    const int st = mb_pcm_check(b, in_bits);
    if (st != PV_OK) return st;
    const MbPcmLayout l = mb_pcm_layout(b, in_bits);
    for (size_t i = 0; i < b->s.size(); ++i) {
        if (in_byte_off) in_byte_off[i] = l.in_off[i];
        if (out_byte_off) out_byte_off[i] = l.out_off[i];
    }
    if (in_bytes) *in_bytes = l.in_bytes;
    if (out_bytes) *out_bytes = l.out_bytes;
    return PV_OK;
}

int pv_mbatch_run_pcm(pv_mbatch *b, const int32_t *in_bits, const void *d_pcm_in, void *d_pcm_out, void *hip_stream) {
    int st = mb_pcm_check(b, in_bits);
    if (st != PV_OK) return st;
    if (!d_pcm_in || (!d_pcm_out && b->out_floats > 0) || (((uintptr_t)d_pcm_in | (uintptr_t)d_pcm_out) & 15)) {
        g_last_error = "mixed batch PCM: the PCM buffers must be non-null and 16-byte aligned";
        return PV_ERR_INVALID_ARG;
    }
    HIPC(hipSetDevice(b->device));
    if ((st = mb_pcm_prepare(b, in_bits)) != PV_OK) return st;
    const pv_mbatch::Pcm &p = b->pcm;
    const int n = (int)b->s.size();
    hipStream_t hs = (hipStream_t)hip_stream;
    launch_mb_pcm_ingest(p.jobs.p, n, p.in_blocks, d_pcm_in, p.stage.p, hs);
    if ((st = pv_mbatch_run(b, p.stage.p, p.stage.p + p.out_base, hip_stream)) != PV_OK) return st;
    launch_mb_pcm_egress(p.jobs.p + n, n, p.out_blocks, p.stage.p + p.out_base, d_pcm_out, hs);
    HIPC(hipGetLastError());
    return PV_OK;
}

int pv_mbatch_debug_pcm_kernel(pv_mbatch *b, int which, const void *d_pcm_in, void *d_pcm_out, void *hip_stream) {
    g_last_error.clear();
    if (!b || !b->pcm.resident || (which != 0 && which != 1) || (which == 0 ? !d_pcm_in : !d_pcm_out) ||
        (((uintptr_t)d_pcm_in | (uintptr_t)d_pcm_out) & 15))
        return PV_ERR_INVALID_ARG;
    HIPC(hipSetDevice(b->device));
    const pv_mbatch::Pcm &p = b->pcm;
    const int n = (int)b->s.size();
    if (which == 0) launch_mb_pcm_ingest(p.jobs.p, n, p.in_blocks, d_pcm_in, p.stage.p, (hipStream_t)hip_stream);
    else launch_mb_pcm_egress(p.jobs.p + n, n, p.out_blocks, p.stage.p + p.out_base, d_pcm_out, (hipStream_t)hip_stream);
    HIPC(hipGetLastError());
    return PV_OK;
}

int pv_mbatch_run_pcm_host(pv_mbatch *b, const int32_t *in_bits, const void *h_pcm_in, void *h_pcm_out) {
    int st = mb_pcm_check(b, in_bits);
    if (st != PV_OK) return st;
    if (!h_pcm_in || (!h_pcm_out && b->out_floats > 0)) {
        g_last_error = "mixed batch PCM: null host buffer";
        return PV_ERR_INVALID_ARG;
    }
    HIPC(hipSetDevice(b->device));
    if ((st = mb_pcm_prepare(b, in_bits)) != PV_OK) return st;
    pv_mbatch::Pcm &p = b->pcm;
    if ((size_t)p.in_bytes > p.d_in.n || !p.d_in.p || (size_t)p.out_bytes > p.d_out.n || !p.d_out.p) {
        HIPC(hipDeviceSynchronize());
        if (((size_t)p.in_bytes > p.d_in.n || !p.d_in.p) && (st = p.d_in.alloc((size_t)p.in_bytes)) != PV_OK) return st;
        if (((size_t)p.out_bytes > p.d_out.n || !p.d_out.p) && (st = p.d_out.alloc((size_t)p.out_bytes)) != PV_OK) return st;
        HIPC(hipDeviceSynchronize());
    }
    HIPC(hipMemcpyAsync(p.d_in.p, h_pcm_in, (size_t)p.in_bytes, hipMemcpyHostToDevice, nullptr));
    if ((st = pv_mbatch_run_pcm(b, in_bits, p.d_in.p, p.d_out.p, nullptr)) != PV_OK) return st;
    if (p.out_bytes > 0) HIPC(hipMemcpyAsync(h_pcm_out, p.d_out.p, (size_t)p.out_bytes, hipMemcpyDeviceToHost, nullptr));
    HIPC(hipStreamSynchronize(nullptr));
    return PV_OK;
}

// one clip through a production kernel, from and to host buffers
static int mb_pcm_debug(const void *h_src, size_t src_bytes, void *h_dst, size_t dst_bytes, int32_t bps, int32_t channels,
                        int64_t frames, bool ingest, int device) {
    g_last_error.clear();
    if (channels < 1 || frames < 0 || (frames > 0 && (!h_src || !h_dst))) return PV_ERR_INVALID_ARG;
    if (frames == 0) return PV_OK;
    const int64_t blocks = mb_pcm_blocks(frames, channels);
    if (blocks > 0x7fffffff) return PV_ERR_INVALID_ARG;
    HIPC(hipSetDevice(device));
    DevBuf<char> src, dst;
    DevBuf<MbPcmJob> job;
    int st;
    if ((st = src.alloc(src_bytes)) != PV_OK || (st = dst.alloc(dst_bytes)) != PV_OK || (st = job.alloc(1)) != PV_OK) return st;
    const MbPcmJob jb{0, 0, frames, channels, bps, 0, 0};
    HIPC(hipMemcpy(job.p, &jb, sizeof jb, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(src.p, h_src, src_bytes, hipMemcpyHostToDevice));
    if (ingest) launch_mb_pcm_ingest(job.p, 1, (int)blocks, src.p, reinterpret_cast<float *>(dst.p), nullptr);
    else launch_mb_pcm_egress(job.p, 1, (int)blocks, reinterpret_cast<const float *>(src.p), dst.p, nullptr);
    HIPC(hipGetLastError());
    HIPC(hipMemcpy(h_dst, dst.p, dst_bytes, hipMemcpyDeviceToHost));
    return PV_OK;
}

int pv_debug_pcm_ingest(const void *pcm, int32_t bits, int32_t channels, int64_t frames, float *planar, int device) {
    if (!mb_pcm_depth_ok(bits)) return PV_ERR_INVALID_ARG;
    const size_t samples = (size_t)(frames > 0 && channels > 0 ? frames * channels : 0);
    return mb_pcm_debug(pcm, samples * (size_t)(bits / 8), planar, samples * sizeof(float), bits / 8, channels, frames, true,
                        device);
}

int pv_debug_pcm_egress(const float *planar, int32_t channels, int64_t frames, int16_t *pcm, int device) {
    const size_t samples = (size_t)(frames > 0 && channels > 0 ? frames * channels : 0);
    return mb_pcm_debug(planar, samples * sizeof(float), pcm, samples * 2, 2, channels, frames, false, device);
}

} // extern "C"

// ---------------------------------------------------------------- plane tap (audiomod_pv.h pv_debug_*_planes)
// Every object's Core keeps its planes as rings [rows][TR][HP] / [rows][TR][PKP], slice t of a row in slot t % TR
// (launch_chunk, pool_feed and the mixed batch's builder all set s0 = t0 % TR).  The tap copies one slice of one row to
// the host after the caller has waited for the object's work; it launches nothing.
static void plane_info_of(const Core &c, int64_t begin, int64_t end, pv_plane_info *o) {
    memset(o, 0, sizeof *o);
    if (end - begin > c.TR) begin = end - c.TR;
    o->slice_begin = begin, o->slice_end = end;
    o->hs = c.d.hs;
    o->peak_capacity = c.pkmax;
    o->has_peaks = c.peaks.p && c.npk.p && c.modes.p && c.rot.p ? 1 : 0;
    o->has_chain = c.outphase.p ? 1 : 0;
}

static int read_planes(const Core &c, int64_t row, int64_t t, int64_t begin, int64_t end, float *mag, float *phase,
                       int32_t *npk, int32_t *peaks, int32_t *mode, float *rot, float *outphase) {
    pv_plane_info pi;
    plane_info_of(c, begin, end, &pi);
    if (t < pi.slice_begin || t >= pi.slice_end) {
        g_last_error = "plane tap: slice " + std::to_string(t) + " is not held: the row's readable slices are [" +
                       std::to_string(pi.slice_begin) + ", " + std::to_string(pi.slice_end) + ")";
        return PV_ERR_INVALID_ARG;
    }
    const int64_t plane = row * c.TR + t % c.TR;
    const size_t H = (size_t)c.d.hs + 1;
    if (mag) HIPC(hipMemcpy(mag, c.mag.p + plane * c.HP, H * sizeof(float), hipMemcpyDeviceToHost));
    if (phase) HIPC(hipMemcpy(phase, c.phase.p + plane * c.HP, H * sizeof(float), hipMemcpyDeviceToHost));
    int32_t n = 0, m = kModeProp; // (core mode 0: every step is a per-bin step)
    if (pi.has_peaks) {
        HIPC(hipMemcpy(&n, c.npk.p + plane, sizeof n, hipMemcpyDeviceToHost));
        HIPC(hipMemcpy(&m, c.modes.p + plane, sizeof m, hipMemcpyDeviceToHost));
        if (n < 0 || n > c.pkmax || m < kModeInit || m > kModeLock) {
            g_last_error = "plane tap: slice " + std::to_string(t) + " holds peak count " + std::to_string(n) +
                           " and mode " + std::to_string(m);
            return PV_ERR_HIP;
        }
        if (npk) *npk = n;
        if (mode) *mode = m;
        if (peaks && n > 0) {
            std::vector<uint16_t> pk((size_t)n);
            HIPC(hipMemcpy(pk.data(), c.peaks.p + plane * c.PKP, (size_t)n * sizeof(uint16_t), hipMemcpyDeviceToHost));
            for (int32_t i = 0; i < n; ++i) peaks[i] = pk[(size_t)i];
        }
        if (rot && m == kModeLock && n > 0)
            HIPC(hipMemcpy(rot, c.rot.p + plane * c.PKP, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    }
    if (outphase && pi.has_chain && m != kModeLock)
        HIPC(hipMemcpy(outphase, c.outphase.p + plane * c.HP, (size_t)c.d.hs * sizeof(float), hipMemcpyDeviceToHost));
    return PV_OK;
}

extern "C" {

int pv_debug_batch_plane_info(const pv_batch *b, pv_plane_info *info) {
    if (!b || !info) return PV_ERR_INVALID_ARG;
    plane_info_of(b->core, b->tap_begin, b->tap_end, info);
    return PV_OK;
}
int pv_debug_batch_chain_runs(const pv_batch *b, int32_t launch, int32_t *runs, int32_t *warmups) {
    if (!b || launch < 0 || (size_t)launch >= b->chunks.size()) return PV_ERR_INVALID_ARG;
    const pv_batch::Chunk &ch = b->chunks[(size_t)launch];
    if (runs) *runs = ch.runs;
    if (warmups) *warmups = ch.warm;
    return PV_OK;
}
int pv_debug_batch_planes(pv_batch *b, int32_t stream, int32_t channel, int64_t slice, float *mag, float *phase,
                          int32_t *npk, int32_t *peaks, int32_t *mode, float *rot, float *outphase) {
    g_last_error.clear();
    if (!b || stream < 0 || stream >= b->core.S || channel < 0 || channel >= b->core.C) return PV_ERR_INVALID_ARG;
    HIPC(hipSetDevice(b->core.device));
    HIPC(hipDeviceSynchronize()); // (a batch runs on its caller's stream and on streams of its own)
    return read_planes(b->core, (int64_t)stream * b->core.C + channel, slice, b->tap_begin, b->tap_end, mag, phase, npk,
                       peaks, mode, rot, outphase);
}

int pv_debug_plane_info(const pv_engine *e, pv_plane_info *info) {
    if (!e || !info) return PV_ERR_INVALID_ARG;
    const int64_t end = e->t_base + (int64_t)e->recent.size();
    plane_info_of(e->core, end - e->tap_n, end, info);
    return PV_OK;
}
int pv_debug_planes(pv_engine *e, int32_t channel, int64_t slice, float *mag, float *phase, int32_t *npk, int32_t *peaks,
                    int32_t *mode, float *rot, float *outphase) {
    g_last_error.clear();
    if (!e || channel < 0 || channel >= e->core.C) return PV_ERR_INVALID_ARG;
    if (e->poisoned) return e->poisoned;
    HIPC(hipSetDevice(e->core.device));
    HIPC(hipStreamSynchronize(e->stream));
    const int64_t end = e->t_base + (int64_t)e->recent.size();
    return read_planes(e->core, channel, slice, end - e->tap_n, end, mag, phase, npk, peaks, mode, rot, outphase);
}

int pv_debug_pool_plane_info(const pv_pool *p, int32_t slot, pv_plane_info *info) {
    if (!pool_slot_ok(p, slot) || !info) return PV_ERR_INVALID_ARG;
    const pv_pool::Slot &sl = p->slots[(size_t)slot];
    plane_info_of(p->core, sl.slices - sl.tap_n, sl.slices, info);
    return PV_OK;
}
int pv_debug_pool_planes(pv_pool *p, int32_t slot, int32_t channel, int64_t slice, float *mag, float *phase, int32_t *npk,
                         int32_t *peaks, int32_t *mode, float *rot, float *outphase) {
    g_last_error.clear();
    if (!pool_slot_ok(p, slot) || channel < 0 || channel >= p->core.C) return PV_ERR_INVALID_ARG;
    if (p->poisoned) return p->poisoned;
    HIPC(hipSetDevice(p->core.device));
    HIPC(hipStreamSynchronize(p->stream)); // (device feeds may be in flight)
    const pv_pool::Slot &sl = p->slots[(size_t)slot];
    return read_planes(p->core, (int64_t)slot * p->core.C + channel, slice, sl.slices - sl.tap_n, sl.slices, mag, phase, npk,
                       peaks, mode, rot, outphase);
}

int pv_debug_mbatch_plane_info(const pv_mbatch *b, int32_t stream, pv_plane_info *info) {
    if (!mb_index_ok(b, stream) || !info) return PV_ERR_INVALID_ARG;
    plane_info_of(b->dev->core, 0, b->tap_ran ? (int64_t)b->s[(size_t)stream].plan.slices.size() : 0, info);
    return PV_OK;
}
int pv_debug_mbatch_planes(pv_mbatch *b, int32_t stream, int32_t channel, int64_t slice, float *mag, float *phase,
                           int32_t *npk, int32_t *peaks, int32_t *mode, float *rot, float *outphase) {
    g_last_error.clear();
    if (!mb_index_ok(b, stream) || channel < 0 || channel >= b->dev->core.C) return PV_ERR_INVALID_ARG;
    const Core &c = b->dev->core;
    HIPC(hipSetDevice(c.device));
    HIPC(hipDeviceSynchronize()); // (a mixed batch runs on its caller's stream)
    return read_planes(c, (int64_t)stream * c.C + channel, slice, 0,
                       b->tap_ran ? (int64_t)b->s[(size_t)stream].plan.slices.size() : 0, mag, phase, npk, peaks, mode, rot,
                       outphase);
}

} // extern "C"
