/* audiomod_pv.h -- C ABI of the MI355X-native phase-vocoder engine (libaudiomod_pv.so).
 *
 * This is the drop-in boundary for the phase-vocoder hot path of tangkk/audiomod.  The
 * reference has no C ABI or plugin loader: its callers use the C++
 * class audiomod::phasevocoder (reference include/dafx/phasevocoder.h:42-117) through
 * modbase / modbase_offline (reference include/dafx/modbase.h:26-66,75-126).  The entry
 * points below are what that class binds to underneath (see include/dafx/phasevocoder.h in
 * this repository for the source-compatible class, and INTEGRATION.md for how a reference
 * maintainer swaps it in).  Plain pointers and sizes only; no C++ or torch types; no
 * exceptions cross this boundary -- every call returns a pv_status.
 *
 * Semantics: one engine instance == one FRESH reference process.  The reference keeps
 * DSP state in process-global statics (phasevocoderprocess.cc:380-384,602,716;
 * phasevocoderimpl.cc:46-62, phasevocoderimpl.h:236-238); here that state is per instance.
 */
#ifndef AUDIOMOD_PV_H
#define AUDIOMOD_PV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* mode / coremode values: reference include/dafx/phasevocoder.h:22-36 */
#define PV_MODE_CONSTANT (-1)
#define PV_MODE_NORMAL_SHIFT 0
#define PV_MODE_GENDER_CHANGE 1
#define PV_MODE_FORMANT_PRESERVE 2
#define PV_MODE_VOCODER_ROSENBERG 3
#define PV_MODE_VOCODER_CHORD 4
#define PV_MODE_NORMAL_STRETCH 5
#define PV_MODE_ROBOTIC 6
#define PV_MODE_WHISPER 7
/* Extension, not a value of the reference's enum: pitch shift whose formants are restored by the reference's
 * cepstral formant shift (formantShiftSlice, phasevocoderprocess.cc:925-999, with env_comp = the pitch scale) --
 * code the reference carries but never calls (its call in formantPreserveSlice is commented out, :838).
 * Any fftsize from 128 up (its lifter keeps 60 quefrencies). */
#define PV_MODE_FORMANT_CEPSTRAL 8
#define PV_CORE_NORMAL_PV 0
#define PV_CORE_PHASE_LOCKED 1
#define PV_CORE_INT_RATIO 2

typedef enum pv_status {
    PV_OK = 0,
    PV_ERR_INVALID_ARG = 1,
    PV_ERR_UNSUPPORTED = 2,   /* unknown mode, fftsize above 8192, or a resample ratio whose
                                 per-slice output cap would bind (reference resampler.cc:783) */
    PV_ERR_NO_DEVICE = 3,     /* no usable MI355X / HIP runtime: the product has NO CPU fallback */
    PV_ERR_HIP = 4,           /* a HIP call failed; pv_last_error() has the text */
    PV_ERR_OUTPUT_OVERRUN = 5 /* caller let more than the reference's output ring capacity pile up
                                 (reference phasevocoderprocess.cc:344-364 drops the slice there) */
} pv_status;

/* Constructor arguments of audiomod::phasevocoder (reference include/dafx/phasevocoder.h:54). */
typedef struct pv_config {
    int32_t sample_rate;
    int32_t channels;
    float time_ratio;
    float pitch_semitones;
    int32_t mode;     /* PV_MODE_* */
    int32_t coremode; /* PV_CORE_* */
    int32_t fftsize;  /* rounded up to a power of two like the reference (phasevocoderimpl.cc:177-181) */
    int32_t hopsize;  /* 0 = auto, the only value the reference CLI passes.  A hop above the FFT size: PV_ERR_UNSUPPORTED
                       * at creation; one so small that lrint(hop x time ratio x pitch scale / 2) is 0: PV_ERR_INVALID_ARG
                       * at creation; both with the reason in pv_last_error().  A slice whose shift increment leaves
                       * [1, fftsize]: PV_ERR_UNSUPPORTED from the call that plans it */
} pv_config;

/* Derived constants (reference Impl::calculateSizes, phasevocoderimpl.cc:169-263, and the Speex set-up,
 * resampler.cc:740-770 + resample.c:661-913). */
typedef struct pv_info {
    int32_t fftsize, hop_in, hop_out_nominal, outbuf_capacity;
    float pitch_scale, hs_ratio;
    int32_t int_ratio, resample;
    uint32_t res_num, res_den;
    int32_t res_filt_len, res_oversample, res_interp;
    int64_t slices;        /* slices processed so far */
    int64_t bytes_per_slice; /* algorithmic HBM bytes per slice, SURVEY.md section 8(d): 4*(3N+7H+2s+h) */
} pv_info;

/* Arithmetic of the synthesis side (process-wide setting, read when an engine is created; default PV_ARITH_FAST,
 * or PV_ARITH_EXACT when the environment has AUDIOMOD_PV_EXACT=1).
 *   Everything up to and including the phase propagation -- window, forward FFT, magnitudes, atan2f, peak picking and
 *   matching, the float / double phase chain -- always follows the reference's x86 build operation for operation
 *   (separate multiplies and adds, its libm's atan2f): the propagation is discontinuous in those values, so nothing
 *   short of the same bits is safe there.  Behind it the output is a continuous function of its inputs, and
 *   BASELINE.json's contract is 1e-4 RMS:
 *   PV_ARITH_EXACT  resynthesis, overlap-add, normalisation and resampling also in the reference's operation order
 *                   (bit-identical to the reference except for the sine / cosine of the resynthesis; ROBOTIC mode
 *                   bit-identical end to end);
 *   PV_ARITH_FAST   where a free-form kernel exists -- the plain pitch-shift / stretch modes in every core mode at fft
 *                   512 ... 4096, the formant / gender modes at fft 2048 -- resynthesis, normalisation and resampling may
 *                   fuse multiply-adds, regroup sums, skip phase wraps and use the hardware's sine / cosine
 *                   (measured: 1e-8 ... 5e-8 RMS against the reference).  Such a configuration then always takes the
 *                   fused overlap-add path, in the single-stream engine and in batches of any size alike, so every
 *                   engine runs the same kernels and they agree with each other bit for bit under either setting.
 *                   Every other mode and size computes as PV_ARITH_EXACT. */
#define PV_ARITH_FAST 0
#define PV_ARITH_EXACT 1
int pv_set_arithmetic(int arith);
int pv_get_arithmetic(void);

const char *pv_strerror(int status);
const char *pv_last_error(void);
/* number of visible HIP devices that are gfx950; <= 0 means the library cannot run */
int pv_device_count(void);

/* ----------------------------------------------------------------------------------------------
 * Host planner only (no GPU needed): the reference's data-independent integer behaviour.
 * Feeds `ncalls` blocks of sizes n[i] through the scheduling logic of Impl::processNormal
 * (phasevocoderimpl.cc:340-369), retrieving everything available after each call like the
 * reference CLI (main/main.cc:484-491); writes the per-call availability to avail[i].  If shift /
 * phase are non-NULL they receive the per-slice increments of calculateIncrements
 * (phasevocoderprocess.cc:412-489), up to max_slices; *nslices gets the slice count.
 * -------------------------------------------------------------------------------------------- */
int pv_plan_simulate(const pv_config *cfg, const int32_t *n, int32_t ncalls, int32_t *avail, int32_t *shift,
                     int32_t *phase, int64_t max_slices, int64_t *nslices, pv_info *info);
/* The first n phases WHISPER mode assigns in a fresh reference process (glibc rand() from its default seed;
 * reference phasevocoderprocess.cc:814-822), in draw order: slice-major, channel, bin 0..N/2. */
int pv_plan_whisper_phases(int64_t n, float *out);
/* The data-independent float tables the planner derives for a configuration, for tests and inspection (no GPU
 * needed): PV_TABLE_WINDOW = the Hann window (windowfunc.h:159-169); PV_TABLE_SINC = the Speex Q4 filter table
 * (resample.c:661-775; empty when the configuration does not resample); PV_TABLE_CARRIER = the first `max` samples of
 * the vocoder carrier (gen/rosenberg.cc, rosenbergchord.cc).  Writes min(len, max) floats, returns the table's
 * length (PV_TABLE_CARRIER: max), or a negative pv_status. */
#define PV_TABLE_WINDOW 0
#define PV_TABLE_SINC 1
#define PV_TABLE_CARRIER 2
int64_t pv_plan_table(const pv_config *cfg, int which, float *out, int64_t max);

/* ----------------------------------------------------------------------------------------------
 * Streaming engine: ONE stream of cfg->channels planar channels, host buffers in and out.
 * Replaces phasevocodercore::{processNormal, numsamples_available, retrieve}
 * (reference src/phasevocoder/phasevocoderinterface.h:24-172; phasevocoderimpl.cc:340-369;
 * phasevocoderprocess.cc:1240-1284), i.e. what audiomod::phasevocoder::processInData /
 * getOutData / processBlock call (reference src/phasevocoder/phasevocoder.cc:87-183).
 * -------------------------------------------------------------------------------------------- */
typedef struct pv_engine pv_engine;

int pv_create(const pv_config *cfg, int device, pv_engine **out);
void pv_destroy(pv_engine *e);
/* == processNormal(in, n): in[c] points at n host floats of channel c.  Synchronous. */
int pv_feed(pv_engine *e, const float *const *in, int32_t n);
/* == numsamples_available() */
int32_t pv_available(const pv_engine *e);
/* == retrieve(out, n): copies min(n, available) frames per channel; returns the count (>= 0) */
int32_t pv_retrieve(pv_engine *e, float *const *out, int32_t n);
int pv_get_info(const pv_engine *e, pv_info *info);

/* ----------------------------------------------------------------------------------------------
 * Formant setting: the cepstral envelope shift of PV_MODE_FORMANT_CEPSTRAL (the reference's
 * formantShiftSlice(channel, env_comp)) as a run-time setting of an object of the two plain modes, with the
 * formants moved independently of the pitch.  A stream's setting is off (the default) or on at formant_semitones:
 *   ratio    = formant_semitones == 0 ? 1.0f : (float)pow(2.0, formant_semitones / 12)   (float quotient, double pow,
 *                                                                                         as the pitch scale is made)
 *   env_comp = pitch_scale / ratio                                                        (float quotient)
 * With the knob at 0 env_comp is pv_info.pitch_scale bit for bit -- mode FORMANT_CEPSTRAL's value: formant-preserving
 * shift; at +x the formants move up x semitones, at the pitch's own value they follow the pitch (env_comp 1).  The
 * stage runs for a slice when the setting is on and env_comp != 1.0f (the mode likewise skips it at pitch scale 1),
 * between the phase stage and synthesis, exactly where the mode's launch sits; it rewrites the slice's magnitude plane
 * in place, so the pv_debug_*_planes taps return the shifted magnitudes, as they do for the mode.  With the setting
 * off an object launches what it always launched.  The stage has one arithmetic under either pv_set_arithmetic value.
 * Scope (every entry point, decided before any device call; a refused call changes nothing): cfg.mode NORMAL_SHIFT or
 * NORMAL_STRETCH, anything else PV_ERR_UNSUPPORTED (for FORMANT_CEPSTRAL pv_last_error() says that the mode already
 * fixes it); a non-finite formant_semitones or |formant_semitones| > 48: PV_ERR_INVALID_ARG.  on == 0 ignores the value.
 *   pv_formant_env_comp     : host only: the env_comp of a stream shifted by pitch_semitones with the knob at
 *                             formant_semitones (PV_ERR_INVALID_ARG for NULL, a non-finite pitch, a value out of range)
 *   pv_set_formant          : the slices of later pv_feed calls
 *   pv_batch_set_formant    : one value for the batch; the launches enqueued after the call (pv_batch_run,
 *                             pv_batch_run_span).  Nothing enqueued earlier is waited for or changed
 *   pv_pool_set_formant     : per slot, changeable between feeds: the slices of later pv_pool_feed /
 *                             pv_pool_feed_device calls.  Host state only -- no wait while device feeds are in flight.
 *                             pv_pool_open* starts a slot with the setting off.  A snapshot blob does not carry the
 *                             setting (its format is unchanged): pv_pool_restore leaves the new slot OFF and the caller
 *                             sets it again.  pv_pool_last_launches grows by one for a feed's launch group in which at
 *                             least one listed slot runs the stage; PV_ERR_INVALID_ARG for a slot that is not open
 *   pv_pool_get_formant     : the slot's setting (either pointer may be NULL); formant_semitones reads 0 when off
 *   pv_mbatch_set_formant   : per stream, formant_semitones[nstreams]: NaN = off; NULL = all off.  The slot tables are
 *                             resident on the device: the call synchronises the device (as pv_mbatch_redraw does), writes
 *                             them and recomputes pv_mbatch_kernel_launches (+ 1 per launch group that holds a stream
 *                             running the stage).  pv_mbatch_run, _run_pcm and _run_pcm_host follow.  pv_mbatch_redraw
 *                             resets every stream to off: the object is again what a new one would be
 * -------------------------------------------------------------------------------------------- */
struct pv_batch; /* (the objects of the sections below) */
struct pv_pool;
struct pv_mbatch;
int pv_formant_env_comp(float pitch_semitones, float formant_semitones, float *env_comp);
int pv_set_formant(pv_engine *e, int on, float formant_semitones);
int pv_batch_set_formant(struct pv_batch *b, int on, float formant_semitones);
int pv_pool_set_formant(struct pv_pool *p, int32_t slot, int on, float formant_semitones);
int pv_pool_get_formant(const struct pv_pool *p, int32_t slot, int *on, float *formant_semitones);
int pv_mbatch_set_formant(struct pv_mbatch *b, const float *formant_semitones);

/* ----------------------------------------------------------------------------------------------
 * Voice setting: the WHISPER voice as a run-time, per-stream setting of the many-stream objects of mode ROBOTIC.  The
 * two voices share everything (hop, planner, resampling: the same derived constants) but the phase synthesis gives
 * each bin: 0 (ROBOTIC) or 2 pi rand() / RAND_MAX (WHISPER).  A stream given the WHISPER voice is from then on, bit
 * for bit, a pv_engine / pv_batch of one stream of mode WHISPER with the stream's pitch and time ratio: its own rand()
 * sequence from the default seed, as in one fresh reference process.  The phases are drawn on the device by a
 * generator kernel (glibc's rand() made parallel over a wave); a stream's generator state is 2728 bytes of device
 * memory, whatever its age.  With the setting untouched every object launches exactly what it always launched.
 * Scope (decided before any device call; a refused call changes nothing): objects whose cfg.mode is
 * PV_MODE_ROBOTIC -- pv_pool_create, pv_pool_create_mixed, pv_mbatch_create; anything else PV_ERR_UNSUPPORTED
 * (pv_last_error() says that the voice belongs to ROBOTIC objects).  An unknown voice, a slot that is not open, a NULL
 * object: PV_ERR_INVALID_ARG.  Creating these objects with cfg.mode WHISPER stays refused.
 *   pv_pool_set_voice   : a slot that has processed no slice yet (pv_info.slices == 0); afterwards
 *                         PV_ERR_INVALID_ARG (a change of voice in mid-stream has no reference to be held to).  Host
 *                         state only -- no wait while device feeds are in flight.  pv_pool_open* starts a slot robotic;
 *                         closing and reopening a slot gives a fresh stream.  pv_pool_last_launches grows by one (the
 *                         generator) for a feed's launch group that holds at least one whisper slot; robotic and
 *                         whisper slots share the group's other launches
 *   pv_pool_get_voice   : the slot's voice (NULL allowed)
 *   pv_mbatch_set_voice : per stream, voice[nstreams]; NULL = all robotic.  Every run starts every stream at draw 0,
 *                         so the whisper streams share one table of phases, [slices of the longest of them][channels]
 *                         [fftsize / 2 + 8] floats, drawn by the call itself; the call synchronises the device like
 *                         pv_mbatch_set_formant.  A run launches what it launched before: pv_mbatch_kernel_launches
 *                         does not change.  pv_mbatch_run, _run_pcm and _run_pcm_host follow.  pv_mbatch_redraw resets
 *                         every stream to robotic
 * Snapshots: the blob of a whisper slot has format version 2, reports cfg.mode PV_MODE_WHISPER (pv_pool_blob_info) and
 * carries the slot's generator state; pv_pool_restore accepts it into a ROBOTIC pool only and the slot continues as
 * the uninterrupted WHISPER engine would.  A robotic slot's blob is version 1, byte for byte what it always was.
 * -------------------------------------------------------------------------------------------- */
#define PV_VOICE_ROBOTIC 0
#define PV_VOICE_WHISPER 1
int pv_pool_set_voice(struct pv_pool *p, int32_t slot, int voice);
int pv_pool_get_voice(const struct pv_pool *p, int32_t slot, int *voice);
int pv_mbatch_set_voice(struct pv_mbatch *b, const int32_t *voice);
/* Diagnostics: the generator kernel alone.  One stream from the fresh state; `ncalls` consecutive launches drawing
 * counts[i] phases each (0 ... 2^31 - 1), the state carried in device memory between them; the phases of all launches,
 * concatenated, to out.  Equals pv_plan_whisper_phases(sum of counts) bit for bit. */
int pv_debug_whisper_phases(const int64_t *counts, int32_t ncalls, float *out, int device);

/* ----------------------------------------------------------------------------------------------
 * Carrier setting: the channel vocoder (PV_MODE_VOCODER_ROSENBERG / PV_MODE_VOCODER_CHORD) as a run-time, per-slot
 * setting of the stream pools of mode ROBOTIC.  A slot given carrier ROSENBERG or CHORD is from then on, bit for bit, a
 * pv_engine of that vocoder mode with the slot's own time ratio and pitch under the pool's arithmetic setting: every
 * available / retrieve / out_frames value, every sample, pv_pool_plan_feed, pv_pool_get_info (resample == 0, the
 * vocoder's hop) and the reference's slice dropping.  The slot's derived constants and planner are that engine's own,
 * built when the setting is made.  It is NOT one more voice: a vocoder stream never resamples (the pitch only moves the
 * hop) and its output-ring guard is one hop, so it plans differently from the ROBOTIC stream of the same values.
 * The carrier needs no state: sample n of a voice is table[n mod (period + 1)] of a host-built period table
 * (pv_plan_carrier), so a slot's carrier follows from its sample position alone.  On the device a feed's launch group
 * that holds at least one carrier slot launches 2 kernels more (pv_pool_last_launches): the carrier generator, which
 * writes each such slot's new samples into its row of a carrier ring (positions as in the input ring), and the set's
 * analysis kernel on those rows, into per-slot carrier planes that the group's synthesis reads.  Robotic, whisper and
 * carrier slots share the group's other launches.  Ring and planes are allocated by the first feed that has a carrier
 * slot; a pool that never uses the setting allocates and launches exactly what it always did.
 * Scope (decided before any device call; a refused call changes nothing, pv_last_error() says why):
 *   a NULL pool, a slot that is not open, an unknown carrier                     PV_ERR_INVALID_ARG
 *   a pool whose cfg.mode is not PV_MODE_ROBOTIC                                 PV_ERR_UNSUPPORTED
 *   a slot that has processed a slice (pv_info.slices > 0)                       PV_ERR_INVALID_ARG
 *   a slot whose voice is WHISPER (and pv_pool_set_voice(WHISPER) on a slot
 *   that has a carrier)                                                          PV_ERR_INVALID_ARG
 *   a pool from pv_pool_create whose configuration resamples (pitch other than
 *   0): a uniform pool runs one resampling variant for all slots -- use
 *   pv_pool_create_mixed, which takes the setting for any slot it could open     PV_ERR_UNSUPPORTED
 *   a vocoder stream that needs more of a per-row buffer than the pool sized     PV_ERR_UNSUPPORTED (names the buffer)
 * pv_pool_open* starts a slot at PV_CARRIER_NONE; PV_CARRIER_NONE before the first slice returns the slot to ROBOTIC.
 * Host state only: no wait while device feeds are in flight.  Creating a pool with the vocoder modes stays refused;
 * the mixed batch has no carrier setting (there a carrier would change a stream's plan and output layout).
 * Snapshots: a carrier slot's blob has format version 3 and reports cfg.mode PV_MODE_VOCODER_* (pv_pool_blob_info);
 * its payload is a robotic slot's -- the carrier row is rewritten from the closed form after pv_pool_restore, which
 * accepts the blob into a ROBOTIC pool only (the uniform-pool rule above applies).  Robotic (version 1) and whisper
 * (version 2) blobs stay byte for byte what they are.
 * -------------------------------------------------------------------------------------------- */
#define PV_CARRIER_NONE 0
#define PV_CARRIER_ROSENBERG 1
#define PV_CARRIER_CHORD 2
int pv_pool_set_carrier(struct pv_pool *p, int32_t slot, int carrier);
int pv_pool_get_carrier(const struct pv_pool *p, int32_t slot, int *carrier);
/* host only, no device: `count` carrier samples from absolute sample index `first` (closed form).  Equals
 * pv_plan_table(PV_TABLE_CARRIER) of the matching vocoder configuration from `first` on, bit for bit (NaN where that
 * is NaN: sample rates at which a voice's opening phase has zero length, e.g. 16 kHz).  carrier: ROSENBERG or CHORD;
 * first, count >= 0; out not NULL. */
int pv_plan_carrier(int32_t sample_rate, int carrier, int64_t first, int64_t count, float *out);
/* diagnostics: the carrier kernel alone; njobs windows (first[i], count[i]) in ONE launch, concatenated into out */
int pv_debug_carrier(int32_t sample_rate, int carrier, const int64_t *first, const int32_t *count, int32_t njobs,
                     float *out, int device);

/* ----------------------------------------------------------------------------------------------
 * Stream pool: up to `capacity` independent LIVE streams of one configuration on one device, each
 * with the semantics of a pv_engine (same cfg, same pv_set_arithmetic setting when the pool is
 * created): fed the same blocks and retrieved between calls, a slot returns bit for bit what that
 * engine returns -- every available / retrieve value, every sample, the reference's slice dropping
 * when output piles up included.  One pv_pool_feed serves many slots with ONE launch sequence.
 *   pv_pool_open   : a fresh stream in the lowest free slot (PV_ERR_INVALID_ARG when all are open)
 *   pv_pool_close  : discards the slot's pending output; the slot becomes free
 *   pv_pool_feed   : slots[i] (distinct open slots) gets n[i] >= 0 frames; in[i*C + c] holds channel
 *                    c of slots[i].  Synchronous.  All or nothing: a call that any slot's planner
 *                    refuses changes no slot (pv_last_error() names the slot).
 * Scope: modes NORMAL_SHIFT, GENDER_CHANGE, FORMANT_PRESERVE, NORMAL_STRETCH, ROBOTIC; coremodes
 * 0-2; fftsize 512 ... 4096 (a mixed pool's, below, too).  Anything else returns PV_ERR_UNSUPPORTED from pv_pool_create;
 * capacity < 1 or capacity x channels > 65535 returns PV_ERR_INVALID_ARG (both checked before any
 * device call).  One host thread per pool.
 * -------------------------------------------------------------------------------------------- */
typedef struct pv_pool pv_pool;
int pv_pool_create(const pv_config *cfg, int32_t capacity, int device, pv_pool **out);
void pv_pool_destroy(pv_pool *p);
int32_t pv_pool_capacity(const pv_pool *p);
int pv_pool_open(pv_pool *p, int32_t *slot);
int pv_pool_close(pv_pool *p, int32_t slot);
int pv_pool_feed(pv_pool *p, int32_t count, const int32_t *slots, const float *const *in, const int32_t *n);
int32_t pv_pool_available(const pv_pool *p, int32_t slot);   /* -1: not an open slot */
int32_t pv_pool_retrieve(pv_pool *p, int32_t slot, float *const *out, int32_t n); /* frames copied, -1: bad slot */
int pv_pool_get_info(const pv_pool *p, int32_t slot, pv_info *info);
/* Diagnostics: wall-clock time of the last pv_pool_feed, split into the host's share up to the wait (planning,
 * descriptors, staging, enqueueing the launches) and the wait for the device.  After a pv_pool_feed_device (below),
 * which does not wait: the call's host time and a wait of 0. */
int pv_pool_last_timing(const pv_pool *p, double *host_us, double *wait_us);
/* Kernels launched by the last pv_pool_feed or pv_pool_feed_device (the input scatter and, with int16 on the wire, the
 * egress kernel included). */
int pv_pool_last_launches(const pv_pool *p, int32_t *launches);

/* Device-resident feed: input and output in device memory, float or int16 (PV_WIRE_F32 / PV_WIRE_I16 below), enqueued
 * and not waited for.  For every listed slot the call is pv_pool_feed with the same samples followed by a
 * pv_pool_retrieve of everything available: out_frames[i] is that count, written before the call returns (the count is
 * data-independent: the slot's planner books feed and retrieve at call time); the samples written to d_out are bit for
 * bit what that pair delivers; pv_pool_available is 0 for these slots afterwards.  Plain and mixed pools, either
 * arithmetic setting.
 *   d_in : [count][C][in_pitch]   entry i, channel c: n[i] valid elements from offset 0
 *   d_out: [count][C][out_pitch]  entry i, channel c: out_frames[i] valid elements from offset 0; the rest of a row is
 *          not written
 *   wire : the element type of BOTH buffers, float (PV_WIRE_F32) or int16_t (PV_WIRE_I16); the pitches are in
 *          elements and arbitrary (the kernels store sample by sample: no alignment is required of pitch or base
 *          beyond the element's own).  int16 converts as pv_hostio does, the reference's WAV reader and writer:
 *          in int16 * (1/32768); out saturate(x * 32768, -32768, 32767) truncated toward zero.
 * pv_pool_plan_feed: host only -- the frames each slot would have available after a feed of n[i] frames (for a slot
 *   without pending output: the out_frames[i] of pv_pool_feed_device); changes nothing.
 * Order: the reads of d_in and the writes of d_out are ordered on `hip_stream` (a hipStream_t passed as void*; NULL =
 *   the default stream) -- the pool's internal stream waits for an event recorded on hip_stream at entry, and
 *   hip_stream waits for the pool's work at exit (the rule of pv_batch_run_span), so both buffers may be reused in
 *   stream order as soon as the call returns.  Up to four calls are in flight; a further one first waits on the host
 *   for the oldest to finish.  pv_pool_feed, pv_pool_open, pv_pool_close and pv_pool_destroy may be called while device
 *   feeds are in flight (pv_pool_feed first waits for them).
 * Host waits: the call does not synchronise, with these exceptions.  A fifth call in flight waits for the oldest (above).
 *   A call that has to GROW one of the pool's buffers (a descriptor block, the int16 arena) frees the old one, which
 *   waits for the device -- the caller's streams included -- and an arena is grown only after the pool's stream has
 *   drained; the buffers start at sizes that serve a few hundred slices per call and double, so this happens a few
 *   times in a pool's life, typically in its first calls.  New buffers are zero-filled on the pool's own stream.
 *   pv_pool_create itself ends with a wait for the default stream (its buffers are zero-filled there).
 * All or nothing, decided before any device call: PV_ERR_INVALID_ARG (pv_last_error() names the slot) for every refusal
 *   of pv_pool_feed, a listed slot that still holds output of pv_pool_feed not yet retrieved, an unknown wire,
 *   n[i] > in_pitch, a planned out_frames[i] > out_pitch, a NULL buffer where a size is positive; a planner's refusal
 *   with the planner's status.  A refused call leaves the pool and out_frames exactly as they were (pv_pool_plan_feed
 *   likewise writes out_frames only when it returns PV_OK).  A launch error that shows only after the call has
 *   returned is reported, and leaves the pool unusable, when its descriptor block is next waited for: by the fourth
 *   pv_pool_feed_device after it, by the next pv_pool_feed, or by a pv_pool_open that uploads a resampling table. */
int pv_pool_plan_feed(pv_pool *p, int32_t count, const int32_t *slots, const int32_t *n, int32_t *out_frames);
int pv_pool_feed_device(pv_pool *p, int32_t count, const int32_t *slots, const int32_t *n, const void *d_in,
                        int64_t in_pitch, void *d_out, int64_t out_pitch, int32_t wire, int32_t *out_frames,
                        void *hip_stream);

/* Mixed pool: slots of one pool at different pitches and time ratios.  cfg fixes sample_rate, channels, mode, coremode,
 * fftsize and hopsize for every slot; a slot opened with pv_pool_open_with(time_ratio, pitch_semitones) is a fresh
 * stream with the semantics of a pv_engine created from cfg with those two values (same pv_set_arithmetic setting as
 * when the pool was created).  pv_pool_open opens a slot at cfg's own values.  Buffers are sized once, at creation,
 * for the whole range.  One feed groups its slots by the kernel variant their engines would run (frequency
 * compensation or not, resampling or not, direct or interpolated table, PV_ARITH_FAST kernels or not) and launches
 * each stage once per variant present, whatever the number of distinct pitches.
 *   pv_pool_create_mixed : range min > max, a NaN, or a range without cfg's values: PV_ERR_INVALID_ARG; out of the pool's
 *                          scope, or a range whose worst case does not fit a per-slot kernel: PV_ERR_UNSUPPORTED
 *                          (pv_last_error() names the kernel).  All checked before any device call.
 *   pv_pool_open_with    : a value outside the pool's range (a pool from pv_pool_create: anything but cfg's values),
 *                          or one the engine itself would refuse, returns an error and changes nothing. */
typedef struct pv_pool_range {
    float min_semitones, max_semitones;   /* pitch_semitones a slot may take */
    float min_time_ratio, max_time_ratio; /* time_ratio a slot may take */
} pv_pool_range;
int pv_pool_create_mixed(const pv_config *cfg, const pv_pool_range *range, int32_t capacity, int device, pv_pool **out);
int pv_pool_open_with(pv_pool *p, float time_ratio, float pitch_semitones, int32_t *slot);

/* Stream pool snapshots: a live slot saved to a blob in host memory and restored into another slot -- of another pool,
 * on another device, in another process, or of the same pool (a fork).  From the restore on, for every sequence of
 * feeds and retrieves, the new slot returns bit for bit what the saved slot returns from the save on: every
 * pv_pool_available value, pv_pool_retrieve count and sample, every out_frames and sample of pv_pool_feed_device, the
 * reference's slice dropping on overrun -- and therefore what an uninterrupted pv_engine returns.
 *   pv_pool_snapshot_bytes : the exact size of the slot's blob in its current state (it depends on the pool's
 *                            configuration and on the slot's pending output, not on the capacity or the slot index);
 *                            -1: not an open slot.
 *   pv_pool_save     : writes one blob per listed slot (distinct, open) into blobs[i], caller-owned host memory of
 *                      capacity[i] bytes, and its size into bytes[i].  Synchronous: it first waits for every
 *                      pv_pool_feed_device in flight, as pv_pool_feed does, gathers the slots' rows of every per-row
 *                      device buffer into the pool's staging buffer with ONE kernel on the pool's stream whatever the
 *                      number of slots, copies the staging buffer to the host with ONE copy, and waits for the stream.
 *                      It leaves every slot exactly as it was (same available, same future output).
 *                      All or nothing: a slot that is not open or listed twice, a capacity below
 *                      pv_pool_snapshot_bytes, a NULL pointer (PV_ERR_INVALID_ARG) or a pool that an earlier failure
 *                      left unusable (its status) are refused before anything is written: no blob, no size.
 *   pv_pool_restore  : opens one fresh slot per blob, lowest free slots first as pv_pool_open does, makes it the saved
 *                      stream and writes its index to slots[i].  One copy of all payloads to the device and ONE kernel
 *                      on the pool's stream, which the call waits for: the restore is ordered before any later feed.
 *                      A mixed pool's table arena is handled as by pv_pool_open_with (an entry shared with an open
 *                      slot of the same ratio, or a free one uploaded).
 *                      All or nothing, decided on the host before any device call and before anything in the pool
 *                      changes (PV_ERR_INVALID_ARG unless stated; pv_last_error() names the blob): fewer free slots
 *                      than blobs; a blob that fails validation; a blob whose stream this pool cannot host.
 *                      The pool must have the geometry and kernels of the pool that saved: sample rate, channels, mode,
 *                      coremode, FFT size, hop setting, the arithmetic setting it was created under, and the derived
 *                      geometry of the per-row buffers (input-ring length, plane-ring slots, plane and peak-list
 *                      pitches, accumulator-ring and stream-ring lengths) -- compared as the two pools' own derived
 *                      values, not as creation arguments; pv_last_error() names the first field that differs.
 *                      Capacity, device and process may differ.  The slot's pitch and time ratio must lie in the pool's
 *                      range (a pool from pv_pool_create: its configuration's own values) and pass the size checks of
 *                      pv_pool_open_with (their status).
 *   pv_pool_blob_info : host only, no device call, works without a GPU: validates a blob and describes it, for a
 *                      router that picks a destination pool.  PV_ERR_INVALID_ARG for NULL, too short or corrupted.
 * pv_pool_last_launches reports 1 after a save or a restore of any number of slots.
 * The blob: little-endian, position-independent; a fixed header (magic, format version, total length, the stream's
 * configuration, its pool's geometry and arithmetic setting, counters), the slot's host state (planner state, the
 * overlap-add builder's live frames, fed / uploaded / slice counters, accumulator half, pending output), the slot's
 * rows of every per-row device buffer, and a 64-bit checksum over all of it (audiomod_amd/csrc/pv_snapshot.h).
 * Validation checks length, magic, version, every internal size against the header's geometry, then the checksum, and
 * never reads past `bytes`.  Two saves of the same stream history are byte-identical, whichever slot or pool the
 * stream ran in and whoever used the slot before: a slot's rows are zeroed when it is opened.
 * A blob is NOT a trust boundary.  Its payload holds peak counts, step modes and ring positions that kernels use as
 * indices; the checksum guards against truncation and accidental corruption, not against a forged blob.  Restore only
 * blobs this library wrote. */
typedef struct pv_pool_blob_desc {
    int32_t version;        /* format version */
    int32_t arithmetic;     /* PV_ARITH_* the saving pool was created under */
    pv_config cfg;          /* the stream's configuration: its pool's, with the slot's own time ratio and pitch */
    float time_ratio, pitch_semitones; /* the slot's own values */
    int64_t slices;         /* slices processed */
    int64_t pending_frames; /* output made and not yet retrieved */
    int64_t payload_bytes;  /* the device rows */
    int64_t total_bytes;
} pv_pool_blob_desc;
int64_t pv_pool_snapshot_bytes(const pv_pool *p, int32_t slot);
int pv_pool_save(pv_pool *p, int32_t count, const int32_t *slots, void *const *blobs, const int64_t *capacity,
                 int64_t *bytes);
int pv_pool_restore(pv_pool *p, int32_t count, const void *const *blobs, const int64_t *bytes, int32_t *slots);
int pv_pool_blob_info(const void *blob, int64_t bytes, pv_pool_blob_desc *info);

/* ----------------------------------------------------------------------------------------------
 * Batch engine: `nstreams` independent streams of identical configuration and length, input and
 * output resident in device memory (HBM).  Equivalent, per stream, to driving the reference CLI
 * loop (main/main.cc:471-510) with `block`-frame calls: flush != 0 -> feed zeros until `frames`
 * output frames exist and truncate to `frames` (pitch-shift modes); flush == 0 -> no flush
 * (time_stretch).  This is the throughput path bench.py measures.
 *   d_in  : [nstreams][channels][frames]      float32, device
 *   d_out : [nstreams][channels][out_frames]  float32, device (out_frames = pv_batch_out_frames)
 * pv_batch_run enqueues all work on `hip_stream` (a hipStream_t passed as void*; NULL = the
 * default stream) and returns without synchronising.
 * -------------------------------------------------------------------------------------------- */
typedef struct pv_batch pv_batch;

int pv_batch_create(const pv_config *cfg, int32_t nstreams, int64_t frames, int32_t block, int32_t flush,
                    int device, pv_batch **out);
void pv_batch_destroy(pv_batch *b);
int64_t pv_batch_out_frames(const pv_batch *b);
int64_t pv_batch_slices(const pv_batch *b); /* slices per channel per stream */
int32_t pv_batch_launches(const pv_batch *b); /* launches of each kernel per pv_batch_run (= chunks of slices) */
/* 1 when pv_batch_run software-pipelines the phase-locked path: the rotation chain (PV_K_SEQ) of chunk i then runs on a
 * second HIP stream beside the synthesis / overlap-add of chunk i-1 and the analysis / match of chunk i+1, so its
 * measured duration overlaps the other kernels' (environment AUDIOMOD_PV_PIPELINE=0 turns it off) */
int32_t pv_batch_pipelined(const pv_batch *b);
int pv_batch_get_info(const pv_batch *b, pv_info *info);
int pv_batch_run(pv_batch *b, const float *d_in, float *d_out, void *hip_stream);
/* Optional per-kernel timing of the NEXT pv_batch_run calls (HIP events on the run's stream).
 * pv_batch_enable_timing(b, n): n = 0 off; n >= 1 instruments every n-th chunk (n = 1: every launch; an event
 * record costs stream time, so full instrumentation slows the run by about 10 %).  After synchronising the
 * stream, pv_batch_kernel_times returns, for each of PV_NUM_KERNELS kernels, the summed device time in ms and
 * the number of instrumented launches since timing was enabled, and resets the accumulation window. */
#define PV_NUM_KERNELS 8
#define PV_K_ANALYZE 0      /* window + forward real FFT + polar (+ peak picking) */
#define PV_K_MATCH 1        /* phase-locked: peak matching, parallel part */
#define PV_K_SEQ 2          /* phase-locked: per-peak rotation chain, sequential over slices */
#define PV_K_PROP 3         /* coremode 0: per-bin phase recurrence */
#define PV_K_SYNTH 4        /* phase application + freqComp + inverse real FFT + window */
#define PV_K_OLA_RESAMPLE 5 /* overlap-add + normalise + resample */
#define PV_K_CEPSTRAL 6     /* PV_MODE_FORMANT_CEPSTRAL: cepstral envelope shift of the magnitudes */
#define PV_K_SYNTH_OLA 7    /* PV_K_SYNTH and PV_K_OLA_RESAMPLE fused: synthesis frames overlap-added in LDS (fft 512 ...
                               4096; the default -- AUDIOMOD_PV_FUSED=0 brings the two separate kernels back) */
int pv_batch_enable_timing(pv_batch *b, int on);
int pv_batch_kernel_times(pv_batch *b, double ms[PV_NUM_KERNELS], int64_t launches[PV_NUM_KERNELS]);
const char *pv_kernel_name(int k);

/* Batch spans: a batch run in TIME segments, so that only a window of every row is in device memory at once.
 * pv_batch_run walks pv_batch_launches() launches of Tc slices per row each, all state carried between them inside
 * the object; a span is a run of consecutive launches [first_launch, first_launch + launches).
 *   pv_batch_plan_spans : host only, like pv_mbatch_layout: the spans of the batch that pv_batch_create(cfg, nstreams,
 *                         frames, block, flush) would build under the current pv_set_arithmetic setting and
 *                         AUDIOMOD_PV_CHUNK_SLICES, cut every `launches_per_span` launches.  Writes min(count, max)
 *                         entries, returns the count or minus a pv_status.  A job without slices has one empty span
 *                         (launches = 0).  NULL cfg, nstreams / frames / block / launches_per_span < 1 (or NULL out
 *                         with max > 0): PV_ERR_INVALID_ARG; a configuration the engine refuses: its status.
 *   pv_batch_span       : the same for an existing batch and an arbitrary span (launches >= 1 inside the batch's).
 * Contract of the ranges (per row, in frames): the out ranges of consecutive spans partition [0, out_frames) in
 * order (empty ranges occur); 0 <= in_begin <= in_end <= frames, in_begin a multiple of 4; begins and ends never
 * decrease from span to span; a merged span's ranges are the hull of its parts'.  [in_begin, in_end) contains
 * [slice_begin * hop, min(frames, (slice_end - 1) * hop + fftsize)) AND everything else the span's kernels load: the
 * analysis kernels fetch the aligned 16-byte pieces that hold a frame plus one more (up to 3 frames before and 4
 * after it), see audiomod_amd/csrc/pv_plan.cc batch_span.  The flush zeros beyond `frames` are never read from memory.
 *   pv_batch_run_span   : runs one span on windows of the rows:
 *       d_in_win : [nstreams][channels][in_pitch],  row r holds input frames [in_begin, in_end) from offset 0
 *       d_out_win: [nstreams][channels][out_pitch], row r receives output frames [out_begin, out_end) from offset 0
 *     pitches in floats, multiples of 4, >= the range's length; bases 16-byte aligned (anything else:
 *     PV_ERR_INVALID_ARG; d_out_win may be NULL when the span's out range is empty, d_in_win when its in range is).
 *     No kernel reads or writes a window outside the reported ranges.
 *     first_launch == 0 starts every stream afresh, as pv_batch_run does; any other value must be the launch after
 *     the previous span's last, otherwise the call returns PV_ERR_INVALID_ARG, enqueues nothing and leaves the
 *     object as it was.  A pv_batch_run in between restarts (the next span must be a first one again).
 *     Enqueues only and returns without synchronising; when it returns, everything the span put on the batch's
 *     internal streams is ordered before later work on `hip_stream`, so both windows may be reused in stream order.
 *     The state a span hands to the next is ordered by that same rule only: consecutive spans go on the same
 *     `hip_stream`, or on streams the caller has ordered himself (the next span's stream waits for an event recorded
 *     behind the previous span) -- nothing inside the object orders two spans on unrelated streams.
 *     For any division of the launches into spans the concatenated outputs are pv_batch_run's, bit for bit.  Inside
 *     a span the launches keep pv_batch_run's order (its software pipeline included); the pipeline drains at the
 *     span's end and the next span starts with its own first analysis, which is what a span costs.
 *     pv_batch_enable_timing instruments pv_batch_run only; spans are never instrumented.
 * What still grows with the length: the per-slice and per-sample descriptors (overlap-add plan, window-sum
 * denominators, resampler tables) are built for the whole job at creation -- about 12-14 bytes of host and device
 * memory per output frame, shared by all streams.  That, not the audio, is the remaining limit on a job's length. */
typedef struct pv_batch_span_info {
    int32_t first_launch, launches;
    int64_t slice_begin, slice_end;   /* slices per row covered */
    int64_t in_begin, in_end;         /* input frames of a row the span's kernels may read  */
    int64_t out_begin, out_end;       /* output frames of a row the span writes             */
} pv_batch_span_info;
int64_t pv_batch_plan_spans(const pv_config *cfg, int32_t nstreams, int64_t frames, int32_t block, int32_t flush,
                            int32_t launches_per_span, pv_batch_span_info *out, int64_t max);
int pv_batch_span(const pv_batch *b, int32_t first_launch, int32_t launches, pv_batch_span_info *out);
int pv_batch_run_span(pv_batch *b, int32_t first_launch, int32_t launches, const float *d_in_win, int64_t in_pitch,
                      float *d_out_win, int64_t out_pitch, void *hip_stream);

/* ----------------------------------------------------------------------------------------------
 * Mixed batch: the batch engine for streams that differ in LENGTH, PITCH and TIME RATIO -- an offline
 * corpus (augmentation with a random shift and stretch per clip, a folder of files) in one object,
 * input and output resident in device memory.  cfg fixes sample_rate, channels, mode, coremode, fftsize
 * and hopsize for every stream; its own time_ratio and pitch_semitones are ignored.  Stream i is, bit
 * for bit, what pv_batch_create(cfg_i, 1, s[i].frames, block, flush) produces, cfg_i being cfg with
 * s[i]'s two values, under the pv_set_arithmetic setting at creation: the reference's slice dropping on
 * output overrun, the flush and the truncation to `frames` apply as they do there.
 *   Packing is tight, no padding (C = cfg->channels):
 *   d_in  : stream i's [C][frames_i]     at float offset in_off[i]  = C * (frames_0 + ... + frames_{i-1})
 *   d_out : stream i's [C][out_frames_i] at float offset out_off[i] = C * (out_frames_0 + ... + out_frames_{i-1})
 * so a caller concatenates its clips and slices the results.
 *   pv_mbatch_layout : host only, no device call: per stream the output length, slice count and the two
 *                      offsets, and the sizes (in floats) of the two packed buffers.  Every output
 *                      pointer may be NULL.
 *   pv_mbatch_create : every stream's constants, plan, overlap-add descriptors and resampler tables are
 *                      built and uploaded here, once (streams with the same Speex rate pair share a
 *                      table; buffers are sized from the actual streams); AUDIOMOD_PV_CHUNK_SLICES and the
 *                      tuning knob AUDIOMOD_PV_CHAIN_RUNS are read here as pv_batch_create reads them.  The
 *                      descriptors are per stream (only streams of equal length, pitch and ratio share
 *                      them): about 14 bytes of host and device memory per output frame and stream, and
 *                      a creation time that grows with the corpus' total length.
 *   pv_mbatch_run    : enqueues all work on `hip_stream` (NULL = the default stream) and returns without
 *                      synchronising; rebuilds nothing on the host.  Every run starts every stream afresh.
 * A run is pv_mbatch_launches() launch groups; group g covers slices [g*Tc, (g+1)*Tc) of every stream
 * that still has slices there (a stream that has ended costs nothing afterwards), and launches each
 * stage once per kernel variant present (frequency compensation or not, resampling or not, direct or
 * interpolated table, PV_ARITH_FAST kernels or not) whatever the number of distinct pitches;
 * pv_mbatch_kernel_launches() is the run's total.
 * Scope: the stream pool's -- modes NORMAL_SHIFT, GENDER_CHANGE, FORMANT_PRESERVE, NORMAL_STRETCH,
 * ROBOTIC; coremodes 0-2; fftsize 512 ... 4096; nstreams x channels <= 65535.
 * Errors, all decided by pv_mbatch_layout and at the top of pv_mbatch_create, before any device call:
 *   outside the scope                                            PV_ERR_UNSUPPORTED, pv_last_error() starts "mixed batch"
 *   nstreams < 1, a frames < 1, block < 1, a NaN or infinite
 *   pitch / time ratio, cfg, s or out NULL                       PV_ERR_INVALID_ARG
 *   a stream whose cfg_i the engine itself refuses               that status; pv_last_error() names the stream index
 *
 * Re-drawing in place (augmentation draws new values every epoch or step):
 *   pv_mbatch_redraw : gives every stream a new length, pitch and time ratio; `s` has pv_mbatch_nstreams(b)
 *                      entries.  cfg, block, flush, the device, the pv_set_arithmetic setting and the two
 *                      environment knobs stay as creation found them (they are not read again).  After PV_OK
 *                      the object is what pv_mbatch_create(cfg, s, nstreams, block, flush, device) would have
 *                      returned: every accessor returns the same value and pv_mbatch_run writes the same bits.
 *                      All or nothing: every check of the table above, the resampler's LDS fit and the
 *                      launchers' limits run before anything in the object changes; a refused redraw returns
 *                      that status and the object runs exactly as before.  (PV_ERR_HIP from an allocation is
 *                      reported the same way; from a copy or kernel after that, the descriptors are undefined.)
 *                      Per-slice and per-tile records are planned on the host; the per-sample arrays
 *                      (window-sum denominators, resampler output tables) are written by two kernels on the
 *                      device.  Buffers grow and never shrink; only a draw whose largest overlap-add advance
 *                      exceeds what the rings were sized for re-initialises the engine core (slow path).
 *                      Synchronises the device before it writes (an earlier pv_mbatch_run may still be in
 *                      flight on any stream) and again before it returns.
 *   pv_mbatch_last_build_timing : the last create or redraw in three parts, microseconds: planning (per-stream
 *                      constants and plans), the other host work up to and including the uploads, and the
 *                      wait for the device build (0 after a create).  Any pointer may be NULL.
 *   pv_mbatch_debug_descriptors : copies one per-stream descriptor array back from the device, at most
 *                      max_bytes of it, and returns its whole length in bytes (or minus a PV_ERR_ status).
 *                      PV_MB_DESC_WDEN: the stream's denominators, launch group after launch group, as the
 *                      kernels read them (reciprocals for a PV_ARITH_FAST stream, padding included);
 *                      PV_MB_DESC_OTAB: its resampler output table, likewise.
 * -------------------------------------------------------------------------------------------- */
typedef struct pv_mbatch_stream {
    int64_t frames;
    float time_ratio;
    float pitch_semitones;
} pv_mbatch_stream;
typedef struct pv_mbatch pv_mbatch;

int pv_mbatch_layout(const pv_config *cfg, const pv_mbatch_stream *s, int32_t nstreams, int32_t block, int32_t flush,
                     int64_t *out_frames, int64_t *slices, int64_t *in_off, int64_t *out_off,
                     int64_t *in_floats, int64_t *out_floats);
int pv_mbatch_create(const pv_config *cfg, const pv_mbatch_stream *s, int32_t nstreams, int32_t block, int32_t flush,
                     int device, pv_mbatch **out);
void pv_mbatch_destroy(pv_mbatch *b);
int32_t pv_mbatch_nstreams(const pv_mbatch *b);
int64_t pv_mbatch_out_frames(const pv_mbatch *b, int32_t i);   /* -1: bad index */
int64_t pv_mbatch_in_offset(const pv_mbatch *b, int32_t i);    /* float offsets into d_in / d_out */
int64_t pv_mbatch_out_offset(const pv_mbatch *b, int32_t i);
int64_t pv_mbatch_in_floats(const pv_mbatch *b);               /* sizes of the two packed buffers */
int64_t pv_mbatch_out_floats(const pv_mbatch *b);
int32_t pv_mbatch_launches(const pv_mbatch *b);                /* launch groups per run */
int32_t pv_mbatch_kernel_launches(const pv_mbatch *b);         /* kernels per run, all groups */
int pv_mbatch_get_info(const pv_mbatch *b, int32_t i, pv_info *info);
int pv_mbatch_run(pv_mbatch *b, const float *d_in, float *d_out, void *hip_stream); /* enqueues, does not synchronise */
int pv_mbatch_redraw(pv_mbatch *b, const pv_mbatch_stream *s);
int pv_mbatch_last_build_timing(const pv_mbatch *b, double *plan_us, double *host_us, double *device_us);
#define PV_MB_DESC_WDEN 0
#define PV_MB_DESC_OTAB 1
int64_t pv_mbatch_debug_descriptors(const pv_mbatch *b, int32_t stream, int which, void *out, int64_t max_bytes);

/* PCM wire of the mixed batch: the clips as WAV files hold them -- interleaved little-endian PCM, [frames_i][C] of
 * 8 (unsigned), 16, 24 or 32 bits in, [out_frames_i][C] of 16 bits out -- converted on the device by two kernels
 * (one launch each per run, whatever the number of clips) with the reference WAV reader's and writer's conversions:
 *   in : 8 bit (p - 128) / 128, 16 bit s / 32768, 24 bit s / 8388608, 32 bit s / 2147483648 rounded to float once
 *   out: saturate(x * 32768, -32768, 32767) truncated toward zero
 * so d_pcm_out holds, for every clip, the writer's conversion of what pv_mbatch_run writes for the reader's
 * conversion of d_pcm_in, bit for bit, under either pv_set_arithmetic setting.
 *   in_bits : [nstreams] 8, 16, 24 or 32 per clip; NULL = 16 for all.  Anything else is PV_ERR_INVALID_ARG, from
 *             every entry below and before any device call.
 *   pv_mbatch_pcm_layout   : host only.  Clip i's input starts at byte in_byte_off[i] and its output at
 *                            out_byte_off[i]: clips lie in stream order, each rounded up to the next multiple of 16
 *                            bytes, so every offset is a multiple of 16; in_bytes / out_bytes are the buffers' sizes
 *                            (padding of the last clip included).  Every output pointer may be NULL.  The layout
 *                            follows the object's current draw (pv_mbatch_redraw changes it).
 *   pv_mbatch_run_pcm      : device buffers, 16-byte aligned.  Enqueues on `hip_stream`: the ingest kernel, exactly
 *                            what pv_mbatch_run enqueues, the egress kernel; does not synchronise, and takes its
 *                            input from whatever was enqueued on that stream before it (pv_mbatch_run's ordering).
 *                            The kernels neither read nor write the padding bytes between clips.  The float buffers
 *                            in between (in_floats + out_floats) and the kernels' job table belong to the object:
 *                            made by the first PCM run, grown -- never shrunk -- when a redraw needs more.  Only a
 *                            call that finds no table for its in_bits (the first one, one with other depths, the
 *                            first after a redraw) or too small a buffer waits for the device and uploads; any
 *                            other call copies nothing from the host and waits for nothing.
 *   pv_mbatch_run_pcm_host : host buffers of in_bytes / out_bytes (page-locked, pv_host_alloc, for the copies to run
 *                            at PCIe rate).  One copy in, the run, one copy out, one wait: synchronous, nothing
 *                            overlaps.  The device PCM buffers belong to the object.  The copy out covers the whole
 *                            buffer: padding bytes of h_pcm_out are overwritten (with zeros). */
int pv_mbatch_pcm_layout(const pv_mbatch *b, const int32_t *in_bits, int64_t *in_byte_off, int64_t *out_byte_off,
                         int64_t *in_bytes, int64_t *out_bytes);
int pv_mbatch_run_pcm(pv_mbatch *b, const int32_t *in_bits, const void *d_pcm_in, void *d_pcm_out, void *hip_stream);
int pv_mbatch_run_pcm_host(pv_mbatch *b, const int32_t *in_bits, const void *h_pcm_in, void *h_pcm_out);
/* Diagnostics: the two production kernels on one clip, from and to host buffers, so that the conversions can be swept
 * value by value: pcm is [frames][channels] (of `bits` bits on the way in, int16 on the way out), planar
 * [channels][frames]. */
int pv_debug_pcm_ingest(const void *pcm, int32_t bits, int32_t channels, int64_t frames, float *planar, int device);
int pv_debug_pcm_egress(const float *planar, int32_t channels, int64_t frames, int16_t *pcm, int device);
/* ... and one of the two kernels alone as the object's last PCM run launched it (which = 0: ingest from d_pcm_in into
 * the object's float buffer; 1: egress from it into d_pcm_out), for timing; PV_ERR_INVALID_ARG before a PCM run. */
int pv_mbatch_debug_pcm_kernel(pv_mbatch *b, int which, const void *d_pcm_in, void *d_pcm_out, void *hip_stream);

/* ----------------------------------------------------------------------------------------------
 * Host-staged many-stream job.  The reference's callers hold their audio in host memory (planar
 * float buffers filled from 16-bit WAV data: main/main.cc:152-162,484-491; main/wavfile.cc:733-755,
 * 1295-1306,1334-1342), so this is the batch engine with the staging included: `nstreams` streams in
 * host memory, processed in groups of `streams_per_group` whose host-to-device copy, kernels and
 * device-to-host copy overlap (three groups in flight on three HIP streams).  On the wire the
 * samples are float32, or int16 exactly as the reference's WAV reader / writer convert them
 * (in: int16 * 1/32768; out: saturate(x * 32768, -32768, 32767) truncated toward zero).
 *   host_in  : [nstreams][channels][frames]      float32 or int16
 *   host_out : [nstreams][channels][out_frames]  same type
 * Both should be page-locked (pv_host_alloc) for the copies to run at PCIe rate and asynchronously.
 * pv_hostio_run is synchronous: it returns when host_out is complete.
 * -------------------------------------------------------------------------------------------- */
/* Diagnostics: the analysis kernels' atan2f (libm's algorithm restated, audiomod_amd/csrc/pv_atan2f.h, device build)
 * evaluated on host arrays of FINITE values -- tests compare it with the C library's atan2f bit for bit. */
int pv_debug_atan2f(const float *y, const float *x, float *out, int64_t n, int device);
/* ... and the polar conversion of the wave-per-frame analysis kernels (FFT.cc:2623-2630 mag = sqrtf(re^2 + im^2),
 * phase = atan2f(im, re): table-driven atan2f, range-tested short division and square root) on FINITE values. */
int pv_debug_polar(const float *im, const float *re, float *phase, float *mag, int64_t n, int device);
/* ... and its short square root against the correctly rounded one on EVERY float whose bit pattern lies in
 * [first_bits, first_bits + count): the number of mismatches and the first offending pattern. */
int pv_debug_sqrt_sweep(uint32_t first_bits, uint64_t count, uint64_t *mismatches, uint32_t *first_bad, int device);

/* Diagnostics: a census of what the launchers chose.  The fused synthesis + overlap-add kernel exists in four sets
 * (batch, uniform pool, mixed pool, mixed batch) of 60 instantiations each; the census counts launches per
 * instantiation ACTUALLY launched, so a test can assert which one it ran instead of re-deriving the choice.
 *   PV_CENSUS_CHAIN    : a = NC (fft size / 2: 256 ... 2048), b = kPlainCore (0 / 1 / 2 plain per core mode, 3 =
 *                        frequency compensation phase-locked, -1 = all modes), c = kRes, d = kFast (the template
 *                        argument: 0 for an all-modes launch whatever the arithmetic setting)
 *   PV_CENSUS_RESAMPLE : slot-table resampler (pool / pmix / mb sets): a = free-form kernel, b = interpolated table
 *   PV_CENSUS_RESAMPLE_RUNG : the resampling kernel of all four sets: a = the rung launched (PV_RES_RUNG_*), b =
 *                        interpolated table, c = the launch asked for more than 64 KB of LDS.  The batch set counts the
 *                        batch path, the single-stream engine and the host-staged engine (launch_resample)
 *   PV_CENSUS_ANALYZE  : slot-table analysis (pool / pmix / mb sets): a = NC, b = the two-wave split kernel
 *   PV_CENSUS_PHASE    : the phase-locked stage (core mode 1): a = form (PV_PHASE_FORM_*), b = the ring's depth (4 / 8)
 *                        or, for the forms without a ring, the peaks one lane holds (1 / 3).  The batch set counts the
 *                        batch path and the single-stream engine; c and d are ignored
 *   PV_CENSUS_ANALYSIS_KERNEL : the analysis kernel of all four sets: a = the kernel launched (PV_ANA_KERNEL_*), b = NC
 *                        (fft size / 2: 128 ... 4096).  The batch set counts the batch path and the single-stream
 *                        engine, the vocoder modes' carrier launch included.  Read through the call only: neither
 *                        census file lists it.  PV_CENSUS_ANALYZE stays what it was
 *   PV_CENSUS_CEPSTRAL : the cepstral formant stage of all four sets: a = the kernel launched (PV_CEP_KERNEL_*), b = NC
 *                        (fft size / 2: 128 ... 4096).  The batch set counts the batch path and the single-stream engine
 *                        (mode FORMANT_CEPSTRAL and the formant setting alike).  Read through the call only
 *   PV_CENSUS_VOICE    : launches of the voice setting's generator kernel: `set` = the set it serves (pool, pmix, mb;
 *                        pv_debug_whisper_phases counts under batch with a = 1024), a = NC (fft size / 2: 128 ... 4096);
 *                        b, c and d are ignored.  Read through the call only
 * Process-wide and off by default (a launch then tests one flag).  pv_debug_chain_census(on) clears the counts and
 * switches counting on or off; pv_debug_chain_census_count returns a key's count, -1 for a key that does not exist.
 * If the environment variable AUDIOMOD_PV_CHAIN_CENSUS names a file when the library is loaded, the census is on from
 * the start and the process appends its non-zero keys to that file when it exits, one line per key (child processes
 * inherit the variable and append too).  The PV_CENSUS_RESAMPLE_RUNG keys go to the file that AUDIOMOD_PV_RESAMPLE_CENSUS
 * names, in the same way (it may be the same file): the first file keeps exactly the four kinds it always had. */
#define PV_CENSUS_CHAIN 0
#define PV_CENSUS_RESAMPLE 1
#define PV_CENSUS_ANALYZE 2
#define PV_CENSUS_PHASE 3
#define PV_CENSUS_RESAMPLE_RUNG 4
#define PV_CENSUS_ANALYSIS_KERNEL 5
#define PV_CENSUS_CEPSTRAL 7 /* (6 is no kind: -1 for every key, as for any other number) */
#define PV_CENSUS_VOICE 8
#define PV_CEP_KERNEL_GENERIC 0 /* pv_cepstral_kernel: LDS butterflies, any size */
#define PV_CEP_KERNEL_WAVE 1    /* a slice per wave: pv_cepstral_wave_kernel (fft 2048 / 4096), or inside the stream kernel */
#define PV_CEP_KERNEL_SLOT 2    /* pv_slot_cepstral_wave_kernel: the slot-table sets (fft 512 ... 4096) */
#define PV_ANA_KERNEL_GENERIC 0 /* pv_analyze_kernel: LDS butterflies, any size (fft 256 and 8192) */
#define PV_ANA_KERNEL_WAVE 1    /* a frame per wave (fft 512 ... 4096): pv_analyze_wave_kernel, pv_pool_ / pv_pmix_ / pv_mb_ */
#define PV_ANA_KERNEL_SPLIT 2   /* a 4096-point frame on two waves */
#define PV_ANA_KERNEL_STREAM 3  /* the single-launch stream kernel of the drop-in path */
#define PV_RES_RUNG_REF4 0  /* the reference's operation order, four rows per workgroup (PV_ARITH_EXACT) */
#define PV_RES_RUNG_VEC8 1  /* free-form, vector ALU, eight rows per workgroup */
#define PV_RES_RUNG_VEC16 2 /* ... sixteen rows (AUDIOMOD_PV_RES_MFMA=0 only: the matrix-core kernel fits wherever it does) */
#define PV_RES_RUNG_MFMA 3  /* free-form, f32 matrix cores, sixteen rows: while tables + 16 rows fit 64 KB */
#define PV_RES_RUNG_VEC2 4  /* mixed batch only: free-form with two / four rows for mono / stereo ... 4-channel streams */
#define PV_RES_RUNG_VEC4 5
#define PV_PHASE_FORM_RING 0   /* match kernel, then the chain kernel with an LDS ring of b steps */
#define PV_PHASE_FORM_STEP 1   /* match kernel, then the chain kernel that loads one step ahead, b peaks per lane */
#define PV_PHASE_FORM_FUSED 2  /* match and ring chain in one launch (single-stream engine, pool, mixed pool) */
#define PV_PHASE_FORM_STREAM 3 /* the single-launch stream kernel of the drop-in path */
#define PV_CENSUS_SET_BATCH 0
#define PV_CENSUS_SET_POOL 1
#define PV_CENSUS_SET_PMIX 2
#define PV_CENSUS_SET_MB 3
int pv_debug_chain_census(int on);
int64_t pv_debug_chain_census_count(int kind, int set, int a, int b, int c, int d);
/* ... and, host only (no device needed), the rung of the fused ladder that cfg would get under `arith` (PV_ARITH_*):
 * nc, the predicate's value (kPlainCore), resample (kRes) and fast (kFast) -- by the engine's own route, not a second
 * statement of the rule -- with what engine creation decides beside it: the upper bound of waves per workgroup it
 * sizes the launch by, and whether it uploads the window-sum denominators as reciprocals. */
typedef struct pv_chain_rung {
    int32_t nc, plain_core, resample, fast;
    int32_t wave_bound, reciprocal_wden;
} pv_chain_rung;
int pv_debug_chain_rung(const pv_config *cfg, int arith, pv_chain_rung *out);
/* ... and, host only as well, the resampling kernel a batch of `rows` rows (streams x channels) of cfg would get under
 * `arith`, by the launcher's own function: the Speex rate pair, filter length, oversampling and table kind, the LDS
 * layout (table bytes, floats per staged row), and the rung (PV_RES_RUNG_*) with the LDS bytes it asks for.  A
 * configuration that does not resample returns PV_OK with resample = 0 and rung = -1.  Where the rung's request
 * exceeds what a workgroup can get (160 KB - 512) the fields are filled in, refused = 1, and the call returns
 * PV_ERR_UNSUPPORTED with the reason engine creation gives in pv_last_error(). */
typedef struct pv_resample_rung {
    int32_t resample, res_num, res_den, filt_len, oversample, interp;
    int32_t tab_bytes, lds_floats, rung, refused;
    int64_t lds_bytes;
} pv_resample_rung;
int pv_debug_resample_rung(const pv_config *cfg, int arith, int32_t rows, pv_resample_rung *out);

/* Diagnostics: a read-only tap on the planes the analysis and the phase stage leave in device memory, for the batch,
 * the single-stream engine, a pool slot and a mixed batch's stream.  Every object keeps them as rings over the slices
 * of a row (one row per stream and channel); a call waits for the object's work (the engine's and the pool's own
 * stream; the whole device for the two batch objects, which run on their caller's stream), copies one slice of one
 * row to the host and launches nothing.
 *   pv_debug_*_plane_info : which slices of a row can be read now, [slice_begin, slice_end) -- the slices of the
 *       object's most recent run (batch: since launch 0, spans included; mixed batch), call that launched any (engine) or
 *       feed that launched any for the slot (pool), as far as the ring holds them: the last ones of a longer run.  Empty
 *       before the first run, after pv_mbatch_redraw, and for a slot just opened or restored.  hs = fft size / 2;
 *       peak_capacity: the most peaks a step lists; has_peaks: the configuration searches peaks and has step modes
 *       (the phase-locked core mode of the modes with a phase recurrence); has_chain: it has an output-phase plane
 *       (core modes 0 and 1 of those modes).  Without either, only mag and phase are returned and the other pointers
 *       are ignored.
 *   pv_debug_*_planes : for slice `slice` of the row, into every non-null pointer:
 *       mag, phase   hs + 1 floats each, as the analysis kernel stored them (FORMANT_CEPSTRAL shifts mag in place)
 *       npk, mode    the step's peak count and PV_STEP_INIT / PROP / LOCK
 *       peaks        npk bins (room for peak_capacity)
 *       rot          a locked step's npk rotations (room for peak_capacity); untouched for any other step
 *       outphase     hs floats for an initial or per-bin step (every step of core mode 0); untouched for a locked one
 *     List slots beyond npk hold whatever the kernels left there and are not returned.  A slice outside the readable
 *     range is PV_ERR_INVALID_ARG with the range in pv_last_error(); nothing is copied then. */
#define PV_STEP_INIT 0
#define PV_STEP_PROP 1
#define PV_STEP_LOCK 2
typedef struct pv_plane_info {
    int64_t slice_begin, slice_end;
    int32_t hs, peak_capacity, has_peaks, has_chain;
} pv_plane_info;
int pv_debug_batch_plane_info(const pv_batch *b, pv_plane_info *info);
int pv_debug_batch_planes(pv_batch *b, int32_t stream, int32_t channel, int64_t slice, float *mag, float *phase,
                          int32_t *npk, int32_t *peaks, int32_t *mode, float *rot, float *outphase);
int pv_debug_plane_info(const pv_engine *e, pv_plane_info *info);
int pv_debug_planes(pv_engine *e, int32_t channel, int64_t slice, float *mag, float *phase, int32_t *npk, int32_t *peaks,
                    int32_t *mode, float *rot, float *outphase);
int pv_debug_pool_plane_info(const pv_pool *p, int32_t slot, pv_plane_info *info);
int pv_debug_pool_planes(pv_pool *p, int32_t slot, int32_t channel, int64_t slice, float *mag, float *phase, int32_t *npk,
                         int32_t *peaks, int32_t *mode, float *rot, float *outphase);
int pv_debug_mbatch_plane_info(const pv_mbatch *b, int32_t stream, pv_plane_info *info);
int pv_debug_mbatch_planes(pv_mbatch *b, int32_t stream, int32_t channel, int64_t slice, float *mag, float *phase,
                           int32_t *npk, int32_t *peaks, int32_t *mode, float *rot, float *outphase);
/* Diagnostics, host only (reads what pv_batch_create laid out; launches nothing): how launch `launch` (0 ...
 * pv_batch_launches - 1) of a batch splits a row's slices for the fused synthesis + overlap-add kernel -- the number
 * of runs (one workgroup per row and run; 1 on the tile path) and the number of warm-up entries in their lists, the
 * copies of earlier frames a later run re-adds before its own (flag bit 1 of a list entry).  Either pointer may be
 * NULL.  A launch outside the range: PV_ERR_INVALID_ARG. */
int pv_debug_batch_chain_runs(const pv_batch *b, int32_t launch, int32_t *runs, int32_t *warmups);

#define PV_WIRE_F32 0
#define PV_WIRE_I16 1
typedef struct pv_hostio pv_hostio;
int pv_hostio_create(const pv_config *cfg, int32_t nstreams, int64_t frames, int32_t block, int32_t flush, int device,
                     int32_t streams_per_group, int32_t wire, pv_hostio **out);
/* Staging by TIME instead of by stream: ONE batch of all `nstreams` streams, run in segments of
 * `launches_per_segment` launches (pv_batch_run_span) through three window slots.  Per segment a pitched copy brings
 * every row's [in_begin, in_end) up, the span runs, and a pitched copy takes [out_begin, out_end) down, on the same
 * three HIP streams with the same event chaining as the grouped object; int16 is converted on the device, window by
 * window.  Device memory for audio is three windows whatever `frames` is, and the result equals the grouped
 * object's and the device-resident batch's bit for bit.  pv_hostio_run, pv_hostio_out_frames and pv_hostio_destroy
 * serve both kinds of object.  NULL cfg / out, nstreams, frames or launches_per_segment < 1, an unknown wire:
 * PV_ERR_INVALID_ARG, before any device call.
 * The windows are sized from the configuration alone, for the worst case of any span of that many launches (every
 * slice at the largest shift increment the planner may choose, twice the nominal one): the output windows, and with
 * them pv_hostio_staging_bytes, are about twice what a steady job fills.  Copies move the actual ranges only. */
int pv_hostio_create_segmented(const pv_config *cfg, int32_t nstreams, int64_t frames, int32_t block, int32_t flush,
                               int device, int32_t launches_per_segment, int32_t wire, pv_hostio **out);
int64_t pv_hostio_staging_bytes(const pv_hostio *h); /* device bytes of the staging buffers (both kinds of object) */
void pv_hostio_destroy(pv_hostio *h);
int64_t pv_hostio_out_frames(const pv_hostio *h);
int pv_hostio_run(pv_hostio *h, const void *host_in, void *host_out);
void *pv_host_alloc(size_t bytes); /* page-locked host memory (NULL on failure) */
void pv_host_free(void *p);

#ifdef __cplusplus
}
#endif
#endif
