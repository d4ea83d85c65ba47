// pv_kernels.h -- launch interface between the host engine (pv_engine.cc) and the gfx950 kernels
// (pv_kernels.hip).  Plain structs; everything is sized and validated on the host before launch.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace pv {

constexpr int kFftThreads = 256;   // workgroup size of the analysis / synthesis kernels (4 waves)
constexpr int kTileOut = 256;      // outputs (= threads) per workgroup of the OLA+resample kernel
constexpr int kMaxTileFrames = 128; // frames that can overlap one OLA tile (checked on the host; the small FFT
                                    // sizes with a large pitch scale reach ~70 at the automatic hop)

struct DevTables {
    int N, hs, H, HP, nc, log2nc;
    int nstages;
    int radix[16], log2m[16], fstride[16];
    const int32_t *perm;  // [nc] out -> in
    const int32_t *iperm; // [nc] in -> out
    const float2 *tw_fwd, *tw_inv, *st_fwd, *st_inv;
    const float4 *twl_fwd, *twl_inv; // lane-major twiddles of the wave-FFT passes 1 and 2 (pv_wavefft.h), nc 1024 / 2048
    const float *window; // [N]
    const float *window_sh; // [4][N + 8]: window_sh[d][j] = window[j - d] (0 outside), for 16-byte aligned frame loads
};

// Input addressing: sample `a` (absolute frame index of the stream) of stream s, channel c lives at
//   in[s*stride_s + c*stride_c + (a & mask)]  and reads as 0 when a >= len (zero flush).
struct InAddr {
    const float *in;
    int64_t stride_s, stride_c;
    uint64_t mask;
    int64_t len;
};

// Slice-indexed planes (mag, phase, peaks, ...) are rings of TR = Tc + 1 slots per (stream, channel) row:
// slot(t) = t % TR, so the last slice of the previous launch stays readable (the phase recurrences look
// one slice back).
enum : int { kModeInit = 0, kModeProp = 1, kModeLock = 2 };

struct AnalyzeArgs {
    DevTables tb;
    InAddr ia;
    int hop;
    int64_t t0; // first slice of this launch
    int s0;     // ring slot of t0 (= t0 % TR, computed on the host: no 64-bit modulo in the kernels)
    int Tn;     // slices in this launch
    int TR;     // ring slots
    int rows;   // S*C
    int PKP;    // pitch of the peak lists
    int find_peaks;
    int split;       // 4096-point frames on two waves each (tb.twl_fwd then holds WF2048S's lane table)
    float *mag;      // [rows][TR][HP]
    float *phase;    // [rows][TR][HP] analysis phase
    uint16_t *peaks; // [rows][TR][PKP]
    int32_t *npk;    // [rows][TR]
};

// what the sequential kernel needs for one spectral peak of a phase-locked step
struct PeakRec {
    float adv;     // (peak_delta_phi * phaseIncrement) / hop
    float a2;      // analysis phase at the peak bin
    float a1;      // previous analysis phase (same channel) at the matched previous peak bin
    uint32_t p1r1; // p1 | (region index of p1 in the previous same-channel step) << 16
};

struct MatchArgs {
    int N, hs, HP, PKP, C, hop, TR, rows, Tn, s0;
    double two_pi_hop;
    int64_t t0;
    const int32_t *phase_inc; // [Tn]
    const float *phase;
    const uint16_t *peaks;
    const int32_t *npk;
    PeakRec *recs;  // [rows][TR][PKP]
    int32_t *modes; // [rows][TR]
};

struct SeqArgs {
    int N, hs, HP, PKP, C, hop, TR, rows, Tn, s0;
    int high_prio; // s_setprio(3): win every issue arbitration (when the chain's result is what everybody waits for)
    int narrow;    // three peaks per lane: a third of the waves per row (to share a CU with the fused kernel)
    double two_pi_hop;
    int64_t t0;
    const int32_t *phase_inc;
    const float *phase;
    const uint16_t *peaks;
    const int32_t *npk;
    const PeakRec *recs;
    const int32_t *modes;
    float *rot;      // [rows][TR][PKP] rotation of each peak region (LOCK steps)
    float *outphase; // [rows][TR][HP]  per-bin output phase (INIT / PROP steps)
    // persistent per-row state
    int32_t *st_kind; // [rows] 0 = zero state, 1 = po_full valid, 2 = lazily locked (st_rot valid)
    float *st_rot;    // [rows][PKP]
    float *st_po;     // [rows][hs]
};

// coremode 0: per-bin recurrence, one thread per bin, streaming over the slices of the launch
struct PropArgs {
    int N, hs, HP, C, hop, TR, rows, Tn, s0;
    double two_pi_hop;
    int64_t t0;
    const int32_t *phase_inc;
    const float *phase;
    float *outphase;
    float *st_pp; // [rows][hs]
    float *st_po; // [rows][hs]
};

struct SynthArgs {
    DevTables tb;
    int hop, C;
    double two_pi_hop;
    int do_freq_comp;
    float freq_comp, fixed_gain, inv_n;
    int robotic;  // output phase = 0
    int passthru; // CONSTANT mode: output phase = analysis phase
    const float *whisper; // WHISPER mode: [Tn][C][HP] phases drawn on the host (else null)
    // channel vocoder: carrier planes [TR][HP] (one row, shared by every stream and channel); band_len < 0 = off
    int voc_band_len;
    const float *cmag;
    const float *cphase;
    int coremode; // 0: phases from outphase; 1: per-step mode (rot / outphase); 2: phase * inc / hop
    int64_t t0;
    int s0;
    int Tn, TR, rows, PKP;
    const int32_t *phase_inc;
    const float *mag;
    const float *phase;
    const float *outphase;
    const uint16_t *peaks;
    const int32_t *npk;
    const int32_t *modes;
    const float *rot;
    float *frames; // [rows][FR][N] ring of windowed synthesis frames
    int FR;        // power of two
};

// One workgroup of the OLA+resample kernel produces outputs [k0, k0+kcnt) of every (stream, channel).
// cepstral formant shift of the magnitude planes (extension mode PV_MODE_FORMANT_CEPSTRAL)
struct CepstralArgs {
    DevTables tb;
    int Tn, TR, rows, s0;
    float env_comp; // the envelope is read at bin lrint(k * env_comp)
    float inv_n;    // float(1.0 / N)
    float *mag;     // [rows][TR][HP], modified in place
};

struct OlaTile {
    int64_t k0;      // first output index (resampled domain, or OLA domain when not resampling)
    int64_t n_lo;    // first OLA-stream sample the tile needs (may be negative: zero history)
    int32_t kcnt;    // outputs in the tile (<= kTileOut)
    int32_t n_cnt;   // OLA samples needed
    int32_t t_first; // first slice whose frame may overlap [n_lo, n_lo+n_cnt)
    int32_t t_cnt;   // number of candidate slices (<= kMaxTileFrames)
    int32_t p_off;   // offset of t_first's entry in the launch's P list
    int32_t pad;
};

struct OlaArgs {
    int N, rows, FR;
    const float *frames;
    const OlaTile *tiles;
    const int64_t *P; // OLA positions of candidate slices, indexed tile.p_off + j
    int ntiles;
    // resampler
    int resample, interp;
    uint32_t num, den;
    int filt_len, oversample;
    const float *sinc;
    int sinc_len;
    const float4 *tab4; // interpolated mode: [oversample][filt_len + 1] expanded coefficient rows
    const float *wacc;  // [ntiles][wacc_pitch]: window-sum denominators of each tile's OLA samples, then (at
                        // float offset otab_off) the tile's output table: per output two 32-bit words,
                        // { x offset in the tile | sub-sample offset << 16, bits of the interpolation fraction }
    int wacc_pitch, otab_off;
    int lds_floats; // capacity of the OLA tile in LDS
    int tab_bytes;  // LDS bytes of the resampler coefficient table (16-byte multiple)
    // output
    float *out;
    int64_t out_stride_row; // floats between consecutive (stream,channel) rows
    int64_t k_base;         // out index = k - k_base
};

// ---------------------------------------------------------------------------------------------------------------
// Fused synthesis + overlap-add ("chain" kernel): one workgroup per (stream, channel) row walks the launch's slices
// in order with the reference's own streaming state -- the output accumulator (synthesiseSlice / writeSlice,
// phasevocoderprocess.cc:1057-1073,1140-1194) as a ring in LDS -- so the synthesis frames never travel through HBM.
// Wave w synthesises slices w, w + W, w + 2W, ... of the row; frames are added into the accumulator strictly in
// slice order (a turn counter in LDS), which keeps the reference's summation order.  What a slice completes,
// [P_t, P_t + adv), is divided by its window sum and is the output (no resampling) or goes to a small per-row ring
// in HBM from which pv_resample_kernel produces the output.  Everything about a slice that does not depend on the
// data is planned on the host, once for all rows.
// ---------------------------------------------------------------------------------------------------------------
struct ChainSlice {
    int32_t acc_pos;  // (P_t mod AR): accumulator-ring position of the frame's first sample
    int32_t str_pos;  // (P_t & smask): stream-ring position of the first sample this slice finalises
    int32_t adv;      // samples finalised after this slice's frame = its shift increment; 0 when the reference
                      // drops the slice (output ring full, phasevocoderprocess.cc:344-364): the frame stays in the
                      // accumulator and the next frame lands on the same position
    int32_t wden_off; // offset of their window-sum denominators in ChainArgs::wden (laid out by ring quads: entry 0
                      // belongs to sample P_t - (P_t mod 4))
    int32_t k_off;    // not resampling: first output (= finalised sample) of the slice, relative to the launch's
    int32_t kcnt;     // ... and how many of its samples are outputs (the CLI truncates the last ones)
    int32_t flags;    // bit 0: channels > 0 do not add this frame (CONSTANT-mode overrun: processOneSliceConstant
                      // returns after channel 0, phasevocoderprocess.cc:139-150); bit 1: warm-up slice of a later
                      // run -- added and finalised like any other, but its samples are not emitted
    int32_t tl;       // which slice of the launch this is (planes, frame ring)
};

struct ChainArgs {
    int N, rows, C, Tn;
    int AR;     // accumulator ring (floats, multiple of 4, >= N + 4)
    int smask;  // stream ring size - 1 (power of two minus one)
    int waves;  // W: waves per workgroup (= slices of a row in flight)
    int diag;   // always 0 in the product library (a value the compiler cannot see through: pv_kernels.hip
                // PV_CHAIN_DIAG); -DPV_DIAG builds set it from AUDIOMOD_PV_CHAIN_DIAG for elimination timings
    // A row's slices are processed by `runs` workgroups: run r walks slices[run_off[r] .. run_off[r + 1]), a list
    // that begins with the frames before its range whose tails reach into it (flag bit 1: rebuilt, not emitted)
    int runs;
    const int32_t *run_off;   // [runs + 1]
    const ChainSlice *slices; // run lists, concatenated
    const float *wden;        // denominators, indexed wden_off + quad-relative sample
    const float *wden_hi;     // ... for channels > 0 (differs from wden only after a CONSTANT-mode overrun)
    // Ring images carried between launches: two halves of [rows][AR] each.  Run 0 of a row READS half (acc_sel & 1),
    // the row's LAST run WRITES the other half, and the engine flips the bit per launch: with one buffer the last
    // run's workgroup could overwrite the image before a late-starting run 0 of the same launch had read it (nothing
    // orders the workgroups of one launch; seen in round 2 as a rare, deterministic wrong value).  acc_sel bit 1: the
    // launch starts the stream (slice 0) -- the accumulator is all zeros by definition (channelinfo.cc:93-115) and
    // nothing is read.  (One pointer and one int rather than two pointers and a flag: the fused kernel is short of
    // scalar registers, and three more of them cost it 400 v_readlane reloads.)
    float *st_acc;
    int acc_sel;
    float *stream;            // [rows][smask + 1] normalised overlap-add stream (resampling configurations)
    int resample;
    // output (not resampling)
    float *out;
    int64_t out_stride_row;
    // frame source when the synthesis runs as its own kernel (FFT sizes without a wave-per-frame transform)
    const float *frames; // [rows][FR][N]
    int FR;
    int64_t t0;
    int fast; // host-side only: pick the free-form (PV_ARITH_FAST) kernel where one exists; wden then holds reciprocals
};
bool synth_chain_has_fast(const SynthArgs &s);
// The rung of launch_chain's ladder a configuration gets (s: what Core::synth_variant fills, plus tb.nc and whisper):
// the predicate's value and the launch bounds, in waves, of the kernel the ladder picks for it -- per kernel set,
// `fast` being ChainArgs::fast.  Sizes without a wave transform have no fused synthesis kernel; for them the bound is
// the one Core::init always used with pv_frames_chain_kernel (sixteen waves for a plain configuration, else twelve).
int synth_chain_plain_core(const SynthArgs &s);
int synth_chain_max_waves(const SynthArgs &s, bool fast);

// Diagnostics: a process-wide census of what the launchers chose (include/audiomod_pv.h pv_debug_chain_census*).
// Off by default; a launch then tests one static flag and nothing else.
enum { PV_CENSUS_SETS = 4 }; // PV_CENSUS_SET_BATCH / POOL / PMIX / MB of the C ABI
void chain_census_enable(bool on); // clears the table either way
// kind: PV_CENSUS_CHAIN (a = NC, b = kPlainCore, c = kRes, d = kFast), PV_CENSUS_RESAMPLE (a = fast, b = interpolated),
// PV_CENSUS_ANALYZE (a = NC, b = split), PV_CENSUS_PHASE (a = form, b = ring depth 4 / 8 or, for the forms without a
// ring, peaks per lane 1 / 3), PV_CENSUS_RESAMPLE_RUNG (all four sets: a = rung kResRung*, b = interpolated, c = the
// launch asked for more than 64 KB of LDS), PV_CENSUS_ANALYSIS_KERNEL (all four sets: a = kAnaKernel*, b = NC 128 ...
// 4096), PV_CENSUS_CEPSTRAL (all four sets: a = kCepKernel*, b = NC 128 ... 4096), PV_CENSUS_VOICE (the generator's
// launches: a = NC 128 ... 4096); -1 for a key that does not exist
// The forms of the phase-locked stage (PV_PHASE_FORM_* of the C ABI): match kernel + ring chain kernel; match kernel +
// chain kernel that loads one step ahead (pv_seq_kernel<1>, or <3> with three peaks per lane); match and ring chain in
// one launch; the single-launch stream kernel.  Set: launch_seq / launch_phase / launch_stream count under batch.
enum { kPhaseFormRing = 0, kPhaseFormStep = 1, kPhaseFormFused = 2, kPhaseFormStream = 3, kPhaseForms = 4 };
// Which analysis kernel a launch is (PV_ANA_KERNEL_* of the C ABI): pv_analyze_kernel; a set's wave-per-frame kernel;
// its kernel with a frame on two waves; pv_stream_kernel, which analyses inside the single launch.  launch_analyze
// and launch_stream count under batch, launch_slot_analyze under its set.
enum { kAnaKernelGeneric = 0, kAnaKernelWave = 1, kAnaKernelSplit = 2, kAnaKernelStream = 3, kAnaKernels = 4 };
// Which cepstral kernel a launch is (PV_CEP_KERNEL_* of the C ABI): pv_cepstral_kernel; pv_cepstral_wave_kernel, or its
// role inside pv_stream_kernel; pv_slot_cepstral_wave_kernel.  The first two count under batch, the last under its set.
enum { kCepKernelGeneric = 0, kCepKernelWave = 1, kCepKernelSlot = 2, kCepKernels = 3 };
int64_t chain_census_count(int kind, int set, int a, int b, int c, int d);
void census_voice(int set, int nc); // PV_CENSUS_VOICE (a = NC 128 ... 4096): one generator launch, counted by launch_whisper

// The voice setting's generator (pv_whisper.hip, pv_whisper.h): one wave per job draws the job's phases from its state
// row and leaves the row advanced.  state: rows of kWhisperStatePitch words; out: the phase buffer; jobs: device memory.
struct WhisperJob;
void launch_whisper(uint32_t *state, float *out, const WhisperJob *jobs, int njobs, int census_set, int nc, hipStream_t st);

// The carrier setting's generator (pv_carrier.hip, pv_carrier.h): njobs windows of carrier samples in one launch, grid
// (ceil(max_n / kCarrierThreads), njobs); a.jobs and a.tab: device memory.
struct CarrierArgs;
void launch_carrier(const CarrierArgs &a, int njobs, int max_n, hipStream_t st);

// pv_resample_kernel: one workgroup = 256 outputs of two rows
struct ResTile {
    int64_t k0;   // first output
    int64_t n_lo; // first stream sample its windows need (negative: zero history)
    int32_t kcnt; // outputs in the tile (<= kTileOut)
    int32_t n_cnt; // stream samples it needs
};
struct ResArgs {
    int rows, ntiles, smask;
    const float *stream;
    const ResTile *tiles;
    const uint2 *otab; // [ntiles][kTileOut]: { first tap's offset in the tile | sub-sample offset << 16, fraction bits }
    int interp, filt_len, oversample, sinc_len;
    const float *sinc;
    const float4 *tab4;
    int lds_floats, tab_bytes;
    float *out;
    int64_t out_stride_row, k_base;
    int fast; // arithmetic free within the 1e-4 RMS contract (pv_resample_fast_kernel) instead of the reference's order
};
// The rungs of the resampler's ladders (PV_RES_RUNG_* of the C ABI): pv_resample_kernel (the reference's order, four
// rows per workgroup), pv_resample_fast_kernel with 8 / 16 rows, pv_resample_mfma_kernel; the mixed batch's free-form
// kernel also exists with 2 and 4 rows.  The slot-table sets count their kernels under the same names.
enum { kResRungRef4 = 0, kResRungVec8 = 1, kResRungVec16 = 2, kResRungMfma = 3, kResRungVec2 = 4, kResRungVec4 = 5, kResRungs = 6 };
// What launch_resample launches for a.rows / a.fast / a.tab_bytes / a.lds_floats (nothing else is read, no device is
// needed): the rung, the dynamic LDS it asks for, and whether that fits a workgroup at all (kMaxDynLds).  The launcher
// itself goes by this answer, and so does engine creation, which refuses a configuration whose rung does not fit.
struct ResRung {
    int rung;
    size_t lds_bytes;
    bool fits;
};
ResRung resample_rung(const ResArgs &a);
void launch_resample(const ResArgs &a, hipStream_t st);
bool launch_phase(const MatchArgs &m, const SeqArgs &a, hipStream_t st); // single-stream engine: match + chain in one launch
size_t chain_lds_bytes(const ChainArgs &a, int nc_wave /* 0: frames from HBM */);
void launch_synth_chain(const SynthArgs &s, const ChainArgs &c, hipStream_t st); // nc 1024 / 2048
void launch_frames_chain(const ChainArgs &c, hipStream_t st);                    // any size, frames from HBM

// Everything one streaming call needs, for the single-launch kernel of the drop-in path (pv_stream_kernel): the
// argument blocks of the stages it chains.  coremode: 1 = match + chain, 0 = per-bin propagation, anything else =
// no phase stage (coremode 2 and the modes that bypass it).
struct StreamArgs {
    AnalyzeArgs aa;
    MatchArgs ma;
    SeqArgs qa;
    PropArgs pa;
    CepstralArgs ca;
    SynthArgs sa;
    OlaArgs oa;
    int coremode, cepstral;
};
size_t ola_lds_bytes(const OlaArgs &a, int rows_per_group); // the tile path's overlap-add + resampling kernel
bool stream_kernel_supported(const StreamArgs &s);  // wave-FFT sizes only (nc 1024 / 2048)
void launch_stream(const StreamArgs &s, hipStream_t st);

bool lds_starts_at_zero(); // build invariant of the wave-per-frame analysis kernels (see pv_kernels.hip)
void launch_analyze(const AnalyzeArgs &a, hipStream_t st);
void launch_match(const MatchArgs &a, hipStream_t st);
void launch_seq(const SeqArgs &a, hipStream_t st);
void launch_prop(const PropArgs &a, hipStream_t st);
void launch_synth(const SynthArgs &a, hipStream_t st);
void launch_cepstral(const CepstralArgs &a, hipStream_t st); // the wave kernel at nc 1024 / 2048, else the generic one
void launch_ola(const OlaArgs &a, hipStream_t st);

// ---------------------------------------------------------------------------------------------------------------
// Stream pool (pv_pool_*): one launch of each stage serves many independent streams ("slots"), each with its own
// schedule.  grid.y (grid.z for the propagation kernel) is the slot's entry in the launch's PoolSlot table; the
// kernels build a slot view of the argument block -- base pointers moved to the slot's C rows, rows = C, the slot's
// t0 / s0 / Tn and descriptors -- and call the batch kernels' device functions.  The argument blocks passed in hold
// the pool-wide base pointers with rows = C.  Buffers whose rows are not [rows][...] are laid out per slot by the
// pool: the accumulator images as [slot][2][C][AR].
// ---------------------------------------------------------------------------------------------------------------
struct PoolSlot {
    int64_t t0;       // the slot's first slice in this launch (its own count)
    int32_t s0, Tn;   // ring slot of t0; the slot's slices in this launch (>= 1)
    int32_t row0;     // first row of the slot (slot index * C)
    int32_t acc_sel;  // ChainArgs::acc_sel of the slot (its own half and "stream starts here" bit)
    int32_t res_ntiles; // tiles of the resampling kernel
    float env_comp;     // the slot's formant setting (pv_slot_cepstral_wave_kernel): CepstralArgs::env_comp, 0 = the
                        // slot does not run the stage
    // byte offsets into the launch's descriptor block (PoolLaunch::desc)
    int64_t pinc_off, cs_off, ro_off, wden_off, res_off, otab_off;
    int64_t out_off;        // float offset of its first output (row 0) in PoolLaunch::out
    int64_t out_stride_row; // floats between its rows there
    int64_t k_base;         // output index of out_off
    int64_t wh_off;         // the voice setting: float offset of the slot's phases [Tn][C][HP] of this launch in
                            // SynthArgs::whisper (drawn by pv_whisper_kernel); -1: the slot stays robotic.  Read only
                            // where the launch's SynthArgs::whisper is set
    int64_t car_off;        // the carrier setting: float offset of the slot's carrier planes [TR][HP] in
                            // SynthArgs::cmag / cphase (written by the group's carrier analysis); -1: none.  Read only
                            // by the pool and pmix sets, and only where the launch's SynthArgs::cmag is set
};
struct PoolLaunch {
    const PoolSlot *slots; // [nslots]
    const char *desc;
    float *out;
    int nslots;
    int max_tn;     // largest Tn of the launch (grid size)
    int max_tiles;  // largest res_ntiles of the launch
};
// input ingest: rows [row0, row0 + C) of the device ring get samples [pos, pos + n) of their stream, channel c read
// from src[src_off + c * src_pitch + i]
struct PoolIngest {
    int64_t src_off, src_pitch, pos;
    int32_t n, row0;
};
// wire: the element type of src (PV_WIRE_F32: float, PV_WIRE_I16: int16_t, converted as the WAV reader does)
void launch_pool_ingest(const void *src, int wire, float *ring, int ring_len, int C, const PoolIngest *ents, int nents,
                        int max_n, hipStream_t st);
// int16 egress of pv_pool_feed_device: channel c of an entry is n floats at arena[src_off + c * src_pitch], converted as
// the WAV writer does into the caller's int16 buffer at dst[dst_off + c * dst_pitch]
struct PoolEgress {
    int64_t src_off, src_pitch, dst_off, dst_pitch;
    int32_t n, pad;
};
void launch_pool_egress_i16(const float *arena, int16_t *dst, int C, const PoolEgress *ents, int nents, int max_n,
                            hipStream_t st);
// Snapshots (pv_pool_save / pv_pool_restore): one launch moves a table of segments between the pool's per-row buffers
// and one contiguous staging buffer.  A segment is `bytes` bytes (a multiple of 4) at bufs[buf] + buf_off on the one side
// and at stage + stage_off on the other; to_stage != 0 gathers into the staging buffer, 0 scatters out of it.  16-byte
// copies where both addresses and the length are multiples of 16, else 4-byte ones.  grid (segments, parts): the parts
// of a segment stride through it together.  The table may live in mapped host memory (each workgroup reads one entry).
constexpr int kSnapBufs = 16;
struct SnapSeg {
    int32_t buf, pad;
    int64_t buf_off, stage_off, bytes;
};
struct SnapArgs {
    char *bufs[kSnapBufs];
    const SnapSeg *segs;
    char *stage;
    int to_stage;
};
void launch_pool_snapshot(const SnapArgs &a, int nsegs, int parts, hipStream_t st);
// Each returns false (launching nothing) when the configuration has no per-slot kernel or it does not fit;
// launch = false: only that check (pv_pool_create asks it once).
bool launch_pool_analyze(const AnalyzeArgs &a, const PoolLaunch &p, hipStream_t st);
// The formant setting's stage for every slot of the table, one launch for all three slot-table sets (census_set: the
// set it counts under).  `a` holds the pool-wide mag base, TR, inv_n and rows = C; Tn, s0 and env_comp come per slot.
bool launch_slot_cepstral(const CepstralArgs &a, const PoolLaunch &p, int census_set, hipStream_t st);
bool pool_phase_supported(int hs, int PKP);
bool launch_pool_phase(const MatchArgs &m, const SeqArgs &a, const PoolLaunch &p, hipStream_t st);
bool launch_pool_prop(const PropArgs &a, const PoolLaunch &p, hipStream_t st);
bool launch_pool_synth_chain(const SynthArgs &s, const ChainArgs &c, const PoolLaunch &p, hipStream_t st,
                             bool launch = true);
bool launch_pool_resample(const ResArgs &a, const PoolLaunch &p, hipStream_t st, bool launch = true);

// Stream pool with per-slot pitch and time ratio (pv_pool_create_mixed): the same stages, each of which also reads its
// slot's entry of a PoolParams table parallel to PoolLaunch::slots (indexed like it) and puts the slot's hop, phase
// advance, frequency compensation, gain and resampler set-up into the slot view.  A launch serves slots of one kernel
// variant (the argument blocks carry the variant's flags: do_freq_comp, resample, interp, fast); the host groups them.
struct PoolParams {
    double two_pi_hop;
    int32_t hop, do_freq_comp;
    float freq_comp, fixed_gain;
    int32_t filt_len, oversample, sinc_len, tab_bytes, lds_floats, pad;
    const float *sinc;  // the slot's Speex table in the pool's table arena (resampling slots)
    const float4 *tab4; // ... and its expanded interpolation rows (interpolating slots)
};
bool launch_pmix_analyze(const AnalyzeArgs &a, const PoolLaunch &p, const PoolParams *q, hipStream_t st);
bool launch_pmix_phase(const MatchArgs &m, const SeqArgs &a, const PoolLaunch &p, const PoolParams *q, hipStream_t st);
bool launch_pmix_prop(const PropArgs &a, const PoolLaunch &p, const PoolParams *q, hipStream_t st);
bool launch_pmix_synth_chain(const SynthArgs &s, const ChainArgs &c, const PoolLaunch &p, const PoolParams *q,
                             hipStream_t st, bool launch = true);
// lds_floats / tab_bytes of `a`: the largest of the launch's slots (the LDS the launch reserves)
bool launch_pmix_resample(const ResArgs &a, const PoolLaunch &p, const PoolParams *q, hipStream_t st, bool launch = true);

// ---------------------------------------------------------------------------------------------------------------
// Mixed batch (pv_mbatch_*): the batch path's long launches with a slot table -- streams of one launch differ in
// length, pitch and time ratio.  A launch group's tables are PoolSlot and PoolParams as in the mixed pool (built once,
// at creation) plus MbSlot, parallel to them.  What differs from the pool's per-slot kernels:
//   - the analysis reads the caller's packed device buffer (slot i: [C][frames_i] at float offset in_off, zeros from
//     frames_i on), not an ingest ring;
//   - a slot has up to the batch path's 512 slices per launch: match and rotation chain are two launches, as there;
//   - the fused synthesis + overlap-add runs one workgroup per (row, run) of a slot, the slot's slices of the launch
//     split into runs by ChainBuilder::end_launch: PoolSlot::ro_off holds runs + 1 offsets into its run lists.
// ---------------------------------------------------------------------------------------------------------------
struct MbSlot {
    int64_t in_off; // float offset of the slot's channel 0 in the caller's input
    int64_t frames; // its length: the channel stride, and where the zero flush starts
    int32_t runs;   // runs of the fused kernel's launch for this slot (>= 1)
    int32_t pad;
};
bool launch_mb_analyze(const AnalyzeArgs &a, const PoolLaunch &p, const PoolParams *q, const MbSlot *m, hipStream_t st);
bool launch_mb_match(const MatchArgs &a, const PoolLaunch &p, const PoolParams *q, hipStream_t st);
bool launch_mb_seq(const SeqArgs &a, const PoolLaunch &p, const PoolParams *q, hipStream_t st);
// max_runs: the largest MbSlot::runs of the launch (grid size)
bool launch_mb_synth_chain(const SynthArgs &s, const ChainArgs &c, const PoolLaunch &p, const PoolParams *q,
                           const MbSlot *m, int max_runs, hipStream_t st, bool launch = true);
// the pool's resampling bodies with as many rows per workgroup as a slot has (a.rows = C)
bool launch_mb_resample(const ResArgs &a, const PoolLaunch &p, const PoolParams *q, hipStream_t st, bool launch = true);

// Descriptor build on the device (pv_mbatch_redraw): one job per (stream, group) and array; every offset is a byte
// offset into the descriptor block.  A job owns the blocks from first_block up to the next job's.
struct MbWdenJob { // PoolSlot::wden_off's array: the window-sum denominators (reciprocals where `fast`)
    int64_t dst_off;
    int64_t p_off, adv_off, woff_off; // the stream's per-slice P (int64), adv and (ChainSlice::wden_off | acc_pos & 3)
                                      // (int32), indexed by the stream's own slice number: coverage reaches back
                                      // across group boundaries
    int32_t t0, Tn;      // the group's slices
    int32_t total;       // entries: the slices' quads and four trailing ones
    int32_t first_block;
    int32_t N, fast;
    float win_gain;
    int32_t pad;
};
struct MbOtabJob { // PoolSlot::otab_off's array: [ntiles][kTileOut] for outputs [ka, kb)
    int64_t dst_off;
    int64_t ka, kb;
    uint32_t res_num, res_den;
    int32_t filt_len, oversample, interp;
    int32_t ntiles, first_block, pad;
};
int mb_build_wden_blocks(int total);
int mb_build_otab_blocks(int ntiles);
void launch_mb_build_wden(const MbWdenJob *jobs, int njobs, int nblocks, char *desc, const float *window, hipStream_t st);
void launch_mb_build_otab(const MbOtabJob *jobs, int njobs, int nblocks, char *desc, hipStream_t st);

// The PCM wire (pv_mbatch_run_pcm): interleaved little-endian PCM clips of differing length <-> the packed planar
// float layout above, one launch each way per run.  One job per clip; a job owns the blocks from first_block up to
// the next job's, one block per kMbPcmTile interleaved samples.  Every clip starts on a 16-byte boundary of the PCM
// buffer (pv_mbatch_pcm_layout), whose base must itself be 16-byte aligned.
struct MbPcmJob {
    int64_t pcm_off;    // byte offset of the clip's [frames][channels] samples
    int64_t planar_off; // float offset of its [channels][frames]
    int64_t frames;
    int32_t channels;
    int32_t bps;        // bytes per sample on the PCM side: 1 ... 4 (ingest), 2 (egress)
    int32_t first_block, pad;
};
int64_t mb_pcm_blocks(int64_t frames, int channels);
void launch_mb_pcm_ingest(const MbPcmJob *jobs, int njobs, int nblocks, const void *pcm, float *planar, hipStream_t st);
void launch_mb_pcm_egress(const MbPcmJob *jobs, int njobs, int nblocks, const float *planar, void *pcm, hipStream_t st);

} // namespace pv
