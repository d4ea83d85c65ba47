// pv_kernels.hip -- hand-written gfx950 (CDNA4, wave64) kernels of the phase-vocoder engine.
//
// Kernels (the HBM-visible stages of SURVEY.md section 8(d); the phase stage is split three ways):
//   pv_analyze_kernel : window -> fftshift -> real FFT (LDS butterflies) -> (mag, phase)
//                       replaces analyzeSlice + FFT::forwardPolar + kiss_fftr
//                       (reference phasevocoderprocess.cc:492-503, FFT.cc:2617-2631, kiss_fftr.c:67-121)
//                       + spectral peak picking of modifySlicePhaseLocked (:587-596)
//   pv_match_kernel   : phase-locked mode, parallel part: peak matching and everything about a peak's
//                       rotation that does not depend on the recurrence (:640-663)
//   pv_seq_kernel     : phase-locked mode, sequential part: the per-peak rotation chain, one workgroup
//                       per (stream, channel) row (:664-665); per-bin INIT / no-peak steps (:606-636)
//   pv_prop_kernel    : coremode 0, per-bin recurrence of modifySliceSimple (:708-753)
//   pv_synth_kernel   : freqComp gather -> mag/N * (cosf, sinf) -> inverse real FFT -> ifftshift * window
//                       replaces freqCompSlice + synthesiseSlice + FFT::inversePolar + kiss_fftri
//                       (phasevocoderprocess.cc:842-923,1001-1075, FFT.cc:2711-2721, kiss_fftr.c:123-159)
//   pv_ola_kernel     : overlap-add gather + window-sum normalisation + Speex Q4 resampling
//                       replaces the accumulate/divide/shift of synthesiseSlice/writeSlice and
//                       resampler::doresample (phasevocoderprocess.cc:1057,1073,1140-1194,
//                       speex/resample.c:353-401,462-560)
//
// Arithmetic contract: this file is compiled with -ffp-contract=off.  Every float expression
// keeps the reference's operand order and rounding points so the FFT, magnitudes, peak picking,
// OLA and resampler MACs are bit-identical to the x86 reference.  The analysis phases are too: atan2f is libm's own
// algorithm (pv_atan2f.h), because the phase propagation is discontinuous in them.  Only the synthesis' sine / cosine
// are approximations of the reference's (pv_sincos.h for wrapped phases, the device libm elsewhere: 1-2 ulp; the output is
// continuous in them).  princarg stays in double with a true IEEE divide, as the reference
// (common/system/sys.h:84,91).
#include "pv_kernels.h"
#include "pv_atan2f.h"
#include "pv_sincos.h"
#include "pv_wavefft.h"
#include "pv_wire.h"
#include "pv_pcm.h"
#include "audiomod_pv.h" // PV_WIRE_*

#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdlib>

namespace pv {

// -DPV_POISON (a debugging build, tools/build_variant.sh poison -DPV_POISON): every kernel first fills its whole
// dynamic LDS with a NaN pattern, and the engine fills every device buffer with 0xFF bytes instead of zeros, so that a
// read of anything the code did not write itself shows up in the output deterministically instead of depending on what
// the CU or the memory held before.  The product build contains none of this.
#ifdef PV_POISON
__device__ __forceinline__ void pv_poison_lds(char *base) {
    const uint32_t bytes = ((const __attribute__((address_space(4))) uint32_t *)__builtin_amdgcn_dispatch_ptr())[7]; // group_segment_size
    const int nt = blockDim.x * blockDim.y * blockDim.z, tid = threadIdx.x;
    for (uint32_t i = tid; i < bytes / 4; i += nt) reinterpret_cast<uint32_t *>(base)[i] = 0x7fc0dead;
    __syncthreads();
}
#define PV_POISON_LDS(base) pv_poison_lds(base)
#else
#define PV_POISON_LDS(base) ((void)0)
#endif

#define PV_PI 3.14159265358979323846

__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
    float2 m;
    m.x = a.x * b.x - a.y * b.y;
    m.y = a.x * b.y + a.y * b.x;
    return m;
}
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

// princarg(a) = mod(a + pi, -2 pi) + pi with mod(x, y) = x - y*floor(x/y), in double (sys.h:84,91), for an argument
// that is a FLOAT (every call site: the sum or difference of float phases, widened).  floor() needs the correctly
// rounded quotient x / y; the divisor is a constant, so the quotient is formed without a division -- q0 = x (1 / y),
// the exact residual r = x - y q0 (fma), q1 = q0 + r (1 / y) (fma) -- and q1 IS the IEEE quotient for every one of
// the 2^32 float arguments: tests/native/host_princarg_all.cc compares it, and the function's result, with the
// reference expression bit for bit on all of them.  Three dependent operations where the division is about ten:
// this is the critical path of the rotation chain's step.
__device__ __forceinline__ double princarg_f(const float af) {
    const double x = (double)af + PV_PI;
    const double y = -2.0 * PV_PI;
    constexpr double inv_y = 1.0 / (-2.0 * PV_PI);
    const double q0 = x * inv_y;
    const double r = __builtin_fma(-y, q0, x);
    const double q1 = __builtin_fma(r, inv_y, q0);
    return (x - (y * floor(q1))) + PV_PI;
}

// atan2f's interval table (pv_atan2f.h) as the kernels read it into LDS
__device__ const PvAtanBlob pv_atan_blob_dev = pv_atan_make_blob();
__device__ __forceinline__ float pv_max3_abs(float a, float b, float c) {
    return __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(a), __builtin_fabsf(b)), __builtin_fabsf(c));
}
__device__ __forceinline__ float pv_min3_abs(float a, float b, float c) {
    return __builtin_fminf(__builtin_fminf(__builtin_fabsf(a), __builtin_fabsf(b)), __builtin_fabsf(c));
}
__device__ __forceinline__ void wave_sync() {
    // LDS operations of one wave execute in issue order; this only stops the compiler from moving LDS
    // accesses across the hand-off between two passes
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// princarg where the argument is the sum or difference of two wrapped phases (|a| <= 2 pi + a few float ulp):
// floor((a + pi) / (-2 pi)) can only be 0, -1 or -2, and which one follows from comparing x = a + pi with 0 and
// 2 pi -- the correctly rounded quotient x / y lies on the same side of 0 and -1 as the exact one (x / 2 pi differs
// from 1 by at least ulp(x) / 2 pi = 1.4e-16, more than half the spacing of doubles around 1) -- and y * n is exact
// for these n.  Bit-identical to princarg_div without the divide (tests/native/host_princarg.cc sweeps it).
__device__ __forceinline__ double princarg_small(double a) {
    const double x = a + PV_PI;
    const double Y = 2.0 * PV_PI;
    const double yn = x > 0.0 ? (x > Y ? 2.0 * Y : Y) : 0.0;
    return (x - yn) + PV_PI;
}

// XCD-aware block -> (row, slice) map: blocks b and b+8 share an XCD (and its L2), so each XCD walks
// whole rows (one stream-channel) slice after slice and re-reads the overlapping input from its own L2.
__device__ __forceinline__ int ring_slot(int s0, int tl, int TR) {
    const int s = s0 + tl; // tl < TR, so one conditional wrap is enough
    return s >= TR ? s - TR : s;
}
__device__ __forceinline__ int ring_prev(int slot, int TR) { return slot == 0 ? TR - 1 : slot - 1; }

__device__ __forceinline__ bool block_to_row_slice(int Tn, int rows, int &row, int &tl) {
    const int b = blockIdx.x;
    const int xcd = b & 7, q = b >> 3;
    row = xcd + 8 * (q / Tn);
    tl = q % Tn;
    return row < rows;
}

// Workgroup size of the generic one-workgroup-per-frame kernels (the sizes without a wave-per-frame transform): a
// 256-point frame is 128 complex points, 32 radix-4 butterflies per stage -- one wave, not four that mostly wait at
// barriers (fft 256 at 128 streams: 1.63 -> 2.17 G samples/s).
static inline int generic_fft_threads(int nc) { return nc <= 128 ? 64 : kFftThreads; }

// Butterfly stages of the half-size complex FFT in LDS, kissfft operation order
// (kf_bfly4 kiss_fft.c:59-103, kf_bfly2 :36-57); stage 0 is the innermost recursion level.
template <bool INV>
__device__ __forceinline__ void fft_stages(float2 *buf, const DevTables &tb, const float2 *__restrict__ tw) {
    const int nt = blockDim.x;
    for (int s = 0; s < tb.nstages; ++s) {
        const int lm = tb.log2m[s], fs = tb.fstride[s];
        const int m = 1 << lm;
        if (tb.radix[s] == 4) {
            const int nb = tb.nc >> 2;
            for (int b = threadIdx.x; b < nb; b += nt) {
                const int k = b & (m - 1);
                const int base = ((b >> lm) << (lm + 2)) + k;
                float2 f0 = buf[base];
                const float2 f1 = buf[base + m], f2 = buf[base + 2 * m], f3 = buf[base + 3 * m];
                const float2 s0 = cmul(f1, tw[k * fs]);
                const float2 s1 = cmul(f2, tw[2 * k * fs]);
                const float2 s2 = cmul(f3, tw[3 * k * fs]);
                const float2 s5 = csub(f0, s1);
                f0 = cadd(f0, s1);
                const float2 s3 = cadd(s0, s2);
                const float2 s4 = csub(s0, s2);
                buf[base + 2 * m] = csub(f0, s3);
                buf[base] = cadd(f0, s3);
                if (INV) {
                    buf[base + m] = make_float2(s5.x - s4.y, s5.y + s4.x);
                    buf[base + 3 * m] = make_float2(s5.x + s4.y, s5.y - s4.x);
                } else {
                    buf[base + m] = make_float2(s5.x + s4.y, s5.y - s4.x);
                    buf[base + 3 * m] = make_float2(s5.x - s4.y, s5.y + s4.x);
                }
            }
        } else {
            const int nb = tb.nc >> 1;
            for (int b = threadIdx.x; b < nb; b += nt) {
                const int k = b & (m - 1);
                const int base = ((b >> lm) << (lm + 1)) + k;
                const float2 f0 = buf[base];
                const float2 t = cmul(buf[base + m], tw[k * fs]);
                buf[base + m] = csub(f0, t);
                buf[base] = cadd(f0, t);
            }
        }
        __syncthreads();
    }
}

// --------------------------------------------------------------------------------------------
// analysis (+ spectral peak picking for the phase-locked mode)
// --------------------------------------------------------------------------------------------
__device__ __forceinline__ bool is_peak(const float *smag, int b, int hs) {
    // modifySlicePhaseLocked (:587-596): strict local maximum over +-2 bins, b in [2, hs-3]
    if (b < 2 || b + 2 >= hs) return false;
    const float mb = smag[b];
    return mb > smag[b - 1] && mb > smag[b - 2] && mb > smag[b + 1] && mb > smag[b + 2];
}

__global__ __launch_bounds__(kFftThreads) void pv_analyze_kernel(const AnalyzeArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    const DevTables &tb = a.tb;
    const int N = tb.N, hs = tb.hs, nc = tb.nc, nt = blockDim.x;
    float2 *buf = reinterpret_cast<float2 *>(smem_raw); // [nc]
    float *smag = reinterpret_cast<float *>(buf + nc);  // [hs + 1]
    int *wcnt = reinterpret_cast<int *>(smag + hs + 4); // [(hs/nt + 1) * 4]
    int row, tl;
    if (!block_to_row_slice(a.Tn, a.rows, row, tl)) return;
    const int64_t t = a.t0 + tl;
    const int slot = ring_slot(a.s0, tl, a.TR);
    const int64_t a0 = t * (int64_t)a.hop;
    // row = s*Cch + c; the host guarantees stride_s == Cch*stride_c for contiguous rows
    const float *__restrict__ in = a.ia.in + (int64_t)row * a.ia.stride_c;
    const float *__restrict__ w = tb.window;

    // windowed, fft-shifted frame packed as nc complex numbers, written in butterfly (permuted) order
    for (int j = threadIdx.x; j < nc; j += nt) {
        const int src = tb.perm[j];
        const int k0 = (2 * src + hs) & (N - 1);
        const int64_t g0 = a0 + k0;
        const float x0 = g0 < a.ia.len ? in[(uint64_t)g0 & a.ia.mask] : 0.f;
        const float x1 = g0 + 1 < a.ia.len ? in[(uint64_t)(g0 + 1) & a.ia.mask] : 0.f;
        buf[j] = make_float2(x0 * w[k0], x1 * w[k0 + 1]);
    }
    __syncthreads();
    fft_stages<false>(buf, tb, tb.tw_fwd);

    // real-FFT split (kiss_fftr.c:91-120) + polar (FFT.cc:2623-2630)
    const int64_t plane = ((int64_t)row * a.TR + slot);
    float *__restrict__ mag = a.mag + plane * tb.HP;
    float *__restrict__ ph = a.phase + plane * tb.HP;
    for (int k = threadIdx.x; k <= nc / 2; k += nt) {
        if (k == 0) {
            const float2 tdc = buf[0];
            const float r0 = tdc.x + tdc.y, rn = tdc.x - tdc.y;
            const float m0 = sqrtf(r0 * r0 + 0.f * 0.f), mn = sqrtf(rn * rn + 0.f * 0.f);
            mag[0] = m0;
            smag[0] = m0;
            ph[0] = pv_atan2f_fd_finite(0.f, r0);
            mag[nc] = mn;
            smag[nc] = mn;
            ph[nc] = pv_atan2f_fd_finite(0.f, rn);
        } else {
            const float2 fpk = buf[k];
            const float2 q = buf[nc - k];
            const float2 fpnk = make_float2(q.x, -q.y);
            const float2 f1k = cadd(fpk, fpnk);
            const float2 f2k = csub(fpk, fpnk);
            const float2 tq = cmul(f2k, tb.st_fwd[k]);
            const float xr = (f1k.x + tq.x) * 0.5f, xi = (f1k.y + tq.y) * 0.5f;
            const float yr = (f1k.x - tq.x) * 0.5f, yi = (tq.y - f1k.y) * 0.5f;
            if (k != nc - k) {
                const float m = sqrtf(xr * xr + xi * xi);
                mag[k] = m;
                smag[k] = m;
                ph[k] = pv_atan2f_fd_finite(xi, xr);
            }
            const float m2 = sqrtf(yr * yr + yi * yi);
            mag[nc - k] = m2;
            smag[nc - k] = m2;
            ph[nc - k] = pv_atan2f_fd_finite(yi, yr);
        }
    }
    if (!a.find_peaks) return;
    __syncthreads();

    // ordered compaction of the peak bins: ballot per 64-bin group, prefix over groups in bin order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = nt >> 6;
    const int J = (hs + nt - 1) / nt;
    for (int j = 0; j < J; ++j) {
        const unsigned long long bm = __ballot(is_peak(smag, threadIdx.x + j * nt, hs));
        if (lane == 0) wcnt[j * nw + wave] = __popcll(bm);
    }
    __syncthreads();
    uint16_t *__restrict__ pk = a.peaks + plane * a.PKP;
    int running = 0, qi = 0;
    for (int j = 0; j < J; ++j) {
        const int mine = j * nw + wave;
        for (; qi < mine; ++qi) running += wcnt[qi];
        const int b = threadIdx.x + j * nt;
        const bool isp = is_peak(smag, b, hs);
        const unsigned long long bm = __ballot(isp);
        if (isp) pk[running + __popcll(bm & ((1ull << lane) - 1ull))] = (uint16_t)b;
    }
    if (threadIdx.x == 0) {
        int total = 0;
        for (int q = 0; q < J * nw; ++q) total += wcnt[q];
        a.npk[plane] = total;
    }
}

// --------------------------------------------------------------------------------------------
// analysis, wave-per-frame variant (N = 2048 / 4096): one 64-lane wave owns a slice, the four waves of a
// workgroup take four consecutive slices of the same row.  No workgroup barrier anywhere.
// --------------------------------------------------------------------------------------------
template <int WPB> __device__ __forceinline__ bool block_to_row_slice_w(int Tn, int rows, int &row, int &tl) {
    const int groups = (Tn + WPB - 1) / WPB;
    const int b = blockIdx.x, xcd = b & 7, q = b >> 3;
    row = xcd + 8 * (q / groups);
    tl = __builtin_amdgcn_readfirstlane(WPB * (q % groups) + (threadIdx.x >> 6)); // wave-uniform: keep it scalar
    return row < rows && tl < Tn;
}

// (the body is a device function of (row, slice) so that the single-launch streaming kernel can call it too)
// ATAB: the LDS address of atan2f's interval table as a compile-time number -- the kernels that call this have no
// static LDS, so their dynamic LDS starts at address 0 (checked on the host: lds_starts_at_zero) and the table's
// offsets fold into the LDS instructions' immediate fields (two vector adds fewer per bin)
template <int NC, uint32_t ATAB>
__device__ __forceinline__ void analyze_wave_role(const AnalyzeArgs &a, const int row, const int tl, cf *lds) {
    typedef __attribute__((address_space(3))) uint32_t lds_u32;
    const unsigned char *atab = reinterpret_cast<const unsigned char *>((uintptr_t)ATAB);
    using W = WF<NC>;
    constexpr int N = 2 * NC, hs = NC, R = W::R;
    const int lane = threadIdx.x & 63;
    // atan2f's interval table (pv_atan2f.h): 256 bytes of LDS behind the waves' regions, (re)written by every wave
    // with the same words before its polar conversion reads them
    const uint32_t atab_word = pv_atan_blob_dev.w[lane];
    const DevTables &tb = a.tb;
    const int64_t t = a.t0 + tl;
    const int slot = ring_slot(a.s0, tl, a.TR);
    const int64_t a0 = t * (int64_t)a.hop;
    const float *__restrict__ in = a.ia.in + (int64_t)row * a.ia.stride_c;
    const float *__restrict__ w = tb.window;
    const cf *__restrict__ tw = reinterpret_cast<const cf *>(tb.tw_fwd);
    const cf *__restrict__ stw = reinterpret_cast<const cf *>(tb.st_fwd);
    const cf2 *__restrict__ twl = reinterpret_cast<const cf2 *>(tb.twl_fwd);

    // Every global load below is issued ahead of its use, as early as the 128-VGPR budget of four waves per SIMD
    // allows (a pass's twiddles while the previous pass finishes, the split's super-twiddles during the last pass,
    // all of them before the first store): a load placed at its use costs the wave a full memory round trip, and one
    // placed after a store also waits for that store to be acknowledged (vmcnt is a single in-order counter).
    WfTw<W> T0, T1, T2;
    wf_load_pass_tw<W, 0>(T0, lane, tw);
    // windowed, fft-shifted frame straight into the pass-0 register layout: for a fixed register the 64
    // lanes read one contiguous 512-byte span of the input (permuted among the lanes)
    cf v[R];
    {
        const int lp = wf_lane_part<W>(0, lane);
        const int lsrc = wf_src_of<W>(lp);
        const uint64_t m0 = (uint64_t)a0 & a.ia.mask;
        if (a0 + N + 4 <= a.ia.len && ((m0 + (uint64_t)(N + 3)) & a.ia.mask) == m0 + (uint64_t)(N + 3)) {
            // The whole frame (and the 16 bytes after it) lies inside the input and does not wrap the ring
            // (wave-uniform, the common case).  Aligned 16-byte loads of the span that contains the frame, times
            // the window copy delayed by the frame's offset d into its first 16 bytes, staged through LDS: nine
            // wide loads of each instead of 48 narrow permuted ones (the texture path is issue-bound), then the
            // pass-0 layout is a pair of adjacent floats per register out of LDS.
            const float *__restrict__ fp = in + m0;
            const uintptr_t fa = reinterpret_cast<uintptr_t>(fp);
            const int d = (int)((fa & 15u) >> 2);
            const float4 *__restrict__ xb = reinterpret_cast<const float4 *>(fa & ~(uintptr_t)15);
            const float4 *__restrict__ wb = reinterpret_cast<const float4 *>(tb.window_sh + (size_t)d * (N + 8));
            constexpr int Q = N / 256; // 16-byte pieces per lane (plus one more on lane 0), eight at a time
            float4 *stage4 = reinterpret_cast<float4 *>(lds);
            float4 xt = make_float4(0.f, 0.f, 0.f, 0.f), wt = xt;
            if (lane == 0) {
                xt = xb[64 * Q];
                wt = wb[64 * Q];
            }
            constexpr int QS = Q < 8 ? Q : 8;
#pragma unroll
            for (int q0 = 0; q0 < Q; q0 += QS) {
                float4 xq[QS], wq[QS];
#pragma unroll
                for (int q = 0; q < QS; ++q) {
                    xq[q] = xb[lane + 64 * (q0 + q)];
                    wq[q] = wb[lane + 64 * (q0 + q)];
                }
#pragma unroll
                for (int q = 0; q < QS; ++q)
                    stage4[lane + 64 * (q0 + q)] =
                        make_float4(xq[q].x * wq[q].x, xq[q].y * wq[q].y, xq[q].z * wq[q].z, xq[q].w * wq[q].w);
            }
            if (lane == 0) stage4[64 * Q] = make_float4(xt.x * wt.x, xt.y * wt.y, xt.z * wt.z, xt.w * wt.w);
            wave_sync();
            const float *stage = reinterpret_cast<const float *>(lds) + d; // stage[k] = x[a0 + k] * w[k]
            const int kl = (2 * lsrc + hs) & (N - 1); // the register part only sets bits the lane part leaves clear
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int kr = 2 * wf_src_of_const<W>(wf_reg_part<W>(0, r));
                const int k0 = kl ^ kr; // == (2 * (lsrc | src_r) + hs) & (N - 1)
                v[r] = cf{stage[k0], stage[k0 + 1]};
            }
            wave_sync();
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int src = lsrc | wf_src_of_const<W>(wf_reg_part<W>(0, r));
                const int k0 = (2 * src + hs) & (N - 1);
                const int64_t g0 = a0 + k0;
                const float x0 = g0 < a.ia.len ? in[(uint64_t)g0 & a.ia.mask] : 0.f;
                const float x1 = g0 + 1 < a.ia.len ? in[(uint64_t)(g0 + 1) & a.ia.mask] : 0.f;
                v[r] = cf{x0 * w[k0], x1 * w[k0 + 1]};
            }
        }
    }
    constexpr int J = NC / 128;
    const int lp0 = wf_lane_part<W>(0, lane), lp1 = wf_lane_part<W>(1, lane), lp2 = wf_lane_part<W>(2, lane);
    WfTwRaw<W, 1> raw1;
    // (PV_EXP_ANA: elimination builds for timing only, results invalid -- bit 0 no butterflies, 1 no LDS exchanges
    // between the passes, 2 no polar conversion, 3 no plane stores, 4 no peak search)
#if defined(PV_EXP_ANA) && (PV_EXP_ANA & 1)
#define PV_ANA_BFLY(x)
#else
#define PV_ANA_BFLY(x) x
#endif
#if defined(PV_EXP_ANA) && (PV_EXP_ANA & 2)
#define PV_ANA_XCHG(x)
#else
#define PV_ANA_XCHG(x) x
#endif
    wf_fetch_pass_tw<W, 1>(raw1, lane, twl);
    PV_ANA_BFLY((wf_apply_pass_stages<W, 0, false>(v, T0)));
    PV_ANA_XCHG((wf_store<W, 0>(lds, v, lp0)));
    wave_sync();
    PV_ANA_XCHG((wf_load<W, 1>(lds, v, lp1)));
    wf_unpack_pass_tw<W, 1>(T1, raw1);
    PV_ANA_BFLY((wf_apply_pass_stages<W, 1, false>(v, T1)));
    WfTwRaw<W, 2> raw2;
    wf_fetch_pass_tw<W, 2>(raw2, lane, twl);
    PV_ANA_XCHG((wf_store<W, 1>(lds, v, lp1)));
    wave_sync();
    PV_ANA_XCHG((wf_load<W, 2>(lds, v, lp2)));
    wf_unpack_pass_tw<W, 2>(T2, raw2);
    PV_ANA_BFLY((wf_apply_pass_stages<W, 2, false>(v, T2)));
    if constexpr (W::NPASS == 4) { // (512 points: the last radix-4 stage is a pass of its own)
        const int lp3 = wf_lane_part<W>(3, lane);
        WfTwRaw<W, 3> raw3;
        wf_fetch_pass_tw<W, 3>(raw3, lane, twl);
        PV_ANA_XCHG((wf_store<W, 2>(lds, v, lp2)));
        wave_sync();
        PV_ANA_XCHG((wf_load<W, 3>(lds, v, lp3)));
        wf_unpack_pass_tw<W, 3>(T2, raw3);
        PV_ANA_BFLY((wf_apply_pass_stages<W, 3, false>(v, T2)));
    }
    cf sw[J];
#pragma unroll
    for (int j = 0; j < J; ++j) sw[j] = stw[lane + 64 * j];
    const cf swmid = stw[NC / 2];
    if constexpr (W::NPASS == 4) wf_store<W, 3>(lds, v, wf_lane_part<W>(3, lane));
    else wf_store<W, 2>(lds, v, lp2);
    wave_sync();

    // real-FFT split (kiss_fftr.c:91-120) + polar (FFT.cc:2623-2630); lane handles k = lane + 64 j and NC - k
    const int64_t plane = ((int64_t)row * a.TR + slot);
    float *__restrict__ mag = a.mag + plane * tb.HP;
    float *__restrict__ ph = a.phase + plane * tb.HP;
    // The split's output bins, cartesian, go back to the wave's LDS region in natural order; the polar conversion
    // then runs as a ROLLED loop over runs of four consecutive bins.  (Unrolled over a lane's 2 J bins it was 2 J
    // inlined copies of atan2f -- libm's algorithm, pv_atan2f.h, ~100 instructions each -- and the 4096-point kernel
    // ran 2.3x slower than with the device library's shorter atan2f; a run of four per iteration keeps four
    // independent evaluations in flight and the phases / magnitudes leave as 16-byte stores.)
    cf xlo[J], xhi[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int k = lane + 64 * j;
        if (j == 0 && lane == 0) {
            const cf tdc = lds[W::pad(0)];
            xlo[0] = cf{tdc.x + tdc.y, 0.f}; // DC and Nyquist: imaginary part forced to 0 (kiss_fftr.c:97-102)
            xhi[0] = cf{tdc.x - tdc.y, 0.f};
        } else {
            const cf fpk = lds[W::pad(k)];
            const cf q = lds[W::pad(NC - k)];
            const cf fpnk = cf{q.x, -q.y};
            const cf f1k = wf_add(fpk, fpnk);
            const cf f2k = wf_sub(fpk, fpnk);
            const cf tq = wf_cmul(f2k, sw[j]);
            xlo[j] = cf{(f1k.x + tq.x) * 0.5f, (f1k.y + tq.y) * 0.5f};
            xhi[j] = cf{(f1k.x - tq.x) * 0.5f, (tq.y - f1k.y) * 0.5f};
        }
    }
    cf xmid = cf{0.f, 0.f};
    if (lane == 0) { // k == NC/2 pairs with itself: the second assignment of the reference loop wins
        const cf fpk = lds[W::pad(NC / 2)];
        const cf fpnk = cf{fpk.x, -fpk.y};
        const cf f1k = wf_add(fpk, fpnk);
        const cf f2k = wf_sub(fpk, fpnk);
        const cf tq = wf_cmul(f2k, swmid);
        xmid = cf{(f1k.x - tq.x) * 0.5f, (tq.y - f1k.y) * 0.5f};
    }
    wave_sync();
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int k = lane + 64 * j;
        if (j == 0 && lane == 0) {
            lds[0] = xlo[0];
            lds[NC] = xhi[0];
        } else {
            lds[k] = xlo[j];
            lds[NC - k] = xhi[j];
        }
    }
    if (lane == 0) lds[NC / 2] = xmid;
    wave_sync();
    // polar (FFT.cc:2623-2630): mag = sqrtf(re^2 + im^2), phase = atan2f(im, re).  The magnitudes also stay in LDS
    // for the peak search: a run's four floats land on the first half of the 32 bytes its cartesian values
    // occupied, and every later run lies beyond them.
    float *smag = reinterpret_cast<float *>(lds);
    *(lds_u32 *)(uintptr_t)(ATAB + 4u * (uint32_t)lane) = atab_word;
    // DC and Nyquist have a zero imaginary part by construction (kiss_fftr.c:97-102): atan2f(+0, r) is +0 or pi by
    // r's sign bit and the magnitude sqrtf(r r + 0 0); lanes 0 and 1 do both at once, and the loop below sees (1, 1)
    // in the DC slot, so that its operand-range test is not tripped by that zero in every frame.
    float edge_mag = 0.f, edge_ph = 0.f;
    if (lane < 2) {
        const cf e = lds[lane == 0 ? 0 : NC];
        edge_mag = sqrtf(e.x * e.x + 0.f * 0.f);
        edge_ph = pv_u2f((uint32_t)((int32_t)pv_f2u(e.x) >> 31) & pv_f2u(3.1415927410e+00f));
    }
    wave_sync();
    if (lane == 0) lds[0] = cf{1.f, 1.f};
    wave_sync();
#pragma nounroll
    for (int q = 0; q < NC / 256; ++q) {
        const int i4 = 4 * (lane + 64 * q);
        const float4 c01 = *reinterpret_cast<const float4 *>(lds + i4);     // bins i4, i4 + 1
        const float4 c23 = *reinterpret_cast<const float4 *>(lds + i4 + 2); // bins i4 + 2, i4 + 3
        float4 m4, p4;
        const float a0 = c01.x * c01.x + c01.y * c01.y, a1 = c01.z * c01.z + c01.w * c01.w;
        const float a2 = c23.x * c23.x + c23.y * c23.y, a3 = c23.z * c23.z + c23.w * c23.w;
        // The short division and square root of pv_atan2f.h need normal operands with magnitudes in [2^-48, 2^63):
        // tested once per run of four bins and wave (true for spectra of audio unless a value is exactly zero --
        // digital silence -- or vanishingly small; the IEEE operations of the other branch serve those).
        const float mx = __builtin_fmaxf(__builtin_fmaxf(pv_max3_abs(c01.x, c01.y, c01.z), pv_max3_abs(c01.w, c23.x, c23.y)),
                                         __builtin_fmaxf(__builtin_fabsf(c23.z), __builtin_fabsf(c23.w)));
        const float mn = __builtin_fminf(__builtin_fminf(pv_min3_abs(c01.x, c01.y, c01.z), pv_min3_abs(c01.w, c23.x, c23.y)),
                                         __builtin_fminf(__builtin_fabsf(c23.z), __builtin_fabsf(c23.w)));
        const bool in_range = mx < 0x1p63f && mn >= 0x1p-48f;
#if defined(PV_EXP_ANA) && (PV_EXP_ANA & 4)
        if (true) {
            m4 = make_float4(a0, a1, a2, a3);
            p4 = make_float4(c01.y + mx, c01.w + mn, c23.y, c23.w);
        } else
#endif
        if (__builtin_amdgcn_ballot_w64(!in_range) == 0) {
            m4 = make_float4(pv_sqrt_safe(a0), pv_sqrt_safe(a1), pv_sqrt_safe(a2), pv_sqrt_safe(a3));
            p4.x = pv_atan2f_fd_tab<true>(c01.y, c01.x, atab);
            p4.y = pv_atan2f_fd_tab<true>(c01.w, c01.z, atab);
            p4.z = pv_atan2f_fd_tab<true>(c23.y, c23.x, atab);
            p4.w = pv_atan2f_fd_tab<true>(c23.w, c23.z, atab);
        } else {
            m4 = make_float4(sqrtf(a0), sqrtf(a1), sqrtf(a2), sqrtf(a3));
            p4.x = pv_atan2f_fd_tab<false>(c01.y, c01.x, atab);
            p4.y = pv_atan2f_fd_tab<false>(c01.w, c01.z, atab);
            p4.z = pv_atan2f_fd_tab<false>(c23.y, c23.x, atab);
            p4.w = pv_atan2f_fd_tab<false>(c23.w, c23.z, atab);
        }
        if (q == 0 && lane == 0) p4.x = edge_ph, m4.x = edge_mag;
#if !(defined(PV_EXP_ANA) && (PV_EXP_ANA & 8))
        *reinterpret_cast<float4 *>(ph + i4) = p4;
        *reinterpret_cast<float4 *>(mag + i4) = m4;
#else
        if (p4.x == 12345.678f) *reinterpret_cast<float4 *>(ph + i4) = p4; // (keeps the values alive)
#endif
        *reinterpret_cast<float4 *>(smag + i4) = m4;
    }
    if (lane == 1) {
        ph[NC] = edge_ph;
        mag[NC] = edge_mag;
        smag[NC] = edge_mag;
    }
    wave_sync();
#if defined(PV_EXP_ANA) && (PV_EXP_ANA & 16)
    if (lane == 0) a.npk[plane] = 100;
    return;
#endif
    if (!a.find_peaks) return;
    // ordered list first into LDS (behind the magnitudes), then out in whole 32-bit words: three coalesced
    // stores per lane instead of one sparsely populated 16-bit store per group of 64 bins
    uint16_t *slist = reinterpret_cast<uint16_t *>(smag + NC + 4); // [PKP], 16-byte aligned
    // A lane tests four consecutive bins (one 16-byte read plus the two bins either side) against the larger of their
    // four neighbours -- is_peak()'s four comparisons as one.  Two peaks are at least three bins apart, so a run of
    // four holds none, one, or its first and last bin: the ordered list position is a prefix count over two lane masks.
    // Bins 0, 1 and hs - 2, hs - 1 are never peaks (:587-596): their outer neighbours read as +infinity.
    int running = 0;
    const float inf = __builtin_inff();
#pragma unroll
    for (int q = 0; q < NC / 256; ++q) {
        const int i4 = 4 * (lane + 64 * q);
        const float4 m = *reinterpret_cast<const float4 *>(smag + i4);
        float2 lo = *reinterpret_cast<const float2 *>(smag + (q == 0 && lane == 0 ? 0 : i4 - 2));
        float2 hi = *reinterpret_cast<const float2 *>(smag + i4 + 4);
        if (q == 0 && lane == 0) lo = make_float2(inf, inf);
        if (q == NC / 256 - 1 && lane == 63) hi = make_float2(inf, inf);
        const float in01 = __builtin_fmaxf(m.x, m.y), in12 = __builtin_fmaxf(m.y, m.z), in23 = __builtin_fmaxf(m.z, m.w);
        const bool f0 = m.x > __builtin_fmaxf(__builtin_fmaxf(lo.x, lo.y), in12);
        const bool f1 = m.y > __builtin_fmaxf(__builtin_fmaxf(lo.y, m.x), in23);
        const bool f2 = m.z > __builtin_fmaxf(in01, __builtin_fmaxf(m.w, hi.x));
        const bool f3 = m.w > __builtin_fmaxf(in12, __builtin_fmaxf(hi.x, hi.y));
        const bool any = f0 || f1 || f2 || f3, two = f0 && f3;
        const unsigned long long ma = __ballot(any), mb = __ballot(two);
        const int pos = running + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(ma >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ma, 0u)) +
                        (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mb >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mb, 0u));
        if (any) slist[pos] = (uint16_t)(i4 + (f0 ? 0 : f1 ? 1 : f2 ? 2 : 3));
        if (two) slist[pos + 1] = (uint16_t)(i4 + 3);
        running += __popcll(ma) + __popcll(mb);
    }
    if (lane == 0) {
        a.npk[plane] = running;
        if (running & 1) slist[running] = 0; // the odd tail shares a word with the last peak
    }
    wave_sync();
    uint32_t *__restrict__ pk32 = reinterpret_cast<uint32_t *>(a.peaks + plane * a.PKP); // PKP % 8 == 0
    const uint32_t *slist32 = reinterpret_cast<const uint32_t *>(slist);
    for (int i = lane; 2 * i < running; i += 64) pk32[i] = slist32[i];
}

// workgroup barrier for hand-overs through LDS: waits for this wave's LDS operations only (a __syncthreads() would also
// wait for its outstanding global stores to be acknowledged)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// The same analysis with a frame on TWO waves (WF2048S: 4096-point frames, 128 lanes x 16 elements): the arithmetic,
// its order and the outputs are those of analyze_wave_role<2048>; what changes is who holds what.  A lane needs the
// registers of the 2048-point frame's kernel (four waves per SIMD instead of two), the passes hand over through workgroup
// barriers, and the peak list's positions need the other wave's counts.  The polar loop overwrites the cartesian bins it
// has consumed with magnitudes, so each of its iterations separates its reads from its writes by a barrier.
template <class W, uint32_t ATAB>
__device__ __forceinline__ void analyze_split_role(const AnalyzeArgs &a, const int row, const int tl, cf *lds) {
    typedef __attribute__((address_space(3))) uint32_t lds_u32;
    const unsigned char *atab = reinterpret_cast<const unsigned char *>((uintptr_t)ATAB);
    constexpr int NC = W::N_C, N = 2 * NC, hs = NC, R = W::R, LN = W::LANES;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t atab_word = pv_atan_blob_dev.w[lane];
    const DevTables &tb = a.tb;
    const int64_t t = a.t0 + tl;
    const int slot = ring_slot(a.s0, tl, a.TR);
    const int64_t a0 = t * (int64_t)a.hop;
    const float *__restrict__ in = a.ia.in + (int64_t)row * a.ia.stride_c;
    const float *__restrict__ w = tb.window;
    const cf *__restrict__ tw = reinterpret_cast<const cf *>(tb.tw_fwd);
    const cf *__restrict__ stw = reinterpret_cast<const cf *>(tb.st_fwd);
    const cf2 *__restrict__ twl = reinterpret_cast<const cf2 *>(tb.twl_fwd);

    WfTw<W> T0, T1, T2;
    wf_load_pass_tw<W, 0>(T0, tid, tw);
    cf v[R];
    {
        const int lp = wf_lane_part<W>(0, tid);
        const int lsrc = wf_src_of<W>(lp);
        const uint64_t m0 = (uint64_t)a0 & a.ia.mask;
        if (a0 + N + 4 <= a.ia.len && ((m0 + (uint64_t)(N + 3)) & a.ia.mask) == m0 + (uint64_t)(N + 3)) {
            // (workgroup-uniform) aligned 16-byte pieces of the span that holds the frame times the window copy delayed
            // by the frame's offset into its first piece, staged through LDS (analyze_wave_role)
            const float *__restrict__ fp = in + m0;
            const uintptr_t fa = reinterpret_cast<uintptr_t>(fp);
            const int d = (int)((fa & 15u) >> 2);
            const float4 *__restrict__ xb = reinterpret_cast<const float4 *>(fa & ~(uintptr_t)15);
            const float4 *__restrict__ wb = reinterpret_cast<const float4 *>(tb.window_sh + (size_t)d * (N + 8));
            constexpr int Q = N / (4 * LN); // 16-byte pieces per lane (plus one more on thread 0)
            float4 *stage4 = reinterpret_cast<float4 *>(lds);
            float4 xt = make_float4(0.f, 0.f, 0.f, 0.f), wt = xt;
            if (tid == 0) {
                xt = xb[LN * Q];
                wt = wb[LN * Q];
            }
            float4 xq[Q], wq[Q];
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                xq[q] = xb[tid + LN * q];
                wq[q] = wb[tid + LN * q];
            }
#pragma unroll
            for (int q = 0; q < Q; ++q)
                stage4[tid + LN * q] = make_float4(xq[q].x * wq[q].x, xq[q].y * wq[q].y, xq[q].z * wq[q].z, xq[q].w * wq[q].w);
            if (tid == 0) stage4[LN * Q] = make_float4(xt.x * wt.x, xt.y * wt.y, xt.z * wt.z, xt.w * wt.w);
            lds_barrier();
            const float *stage = reinterpret_cast<const float *>(lds) + d; // stage[k] = x[a0 + k] * w[k]
            const int kl = (2 * lsrc + hs) & (N - 1);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int kr = 2 * wf_src_of_const<W>(wf_reg_part<W>(0, r));
                const int k0 = kl ^ kr;
                v[r] = cf{stage[k0], stage[k0 + 1]};
            }
            lds_barrier(); // (pass 0 stores over the staged frame)
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int src = lsrc | wf_src_of_const<W>(wf_reg_part<W>(0, r));
                const int k0 = (2 * src + hs) & (N - 1);
                const int64_t g0 = a0 + k0;
                const float x0 = g0 < a.ia.len ? in[(uint64_t)g0 & a.ia.mask] : 0.f;
                const float x1 = g0 + 1 < a.ia.len ? in[(uint64_t)(g0 + 1) & a.ia.mask] : 0.f;
                v[r] = cf{x0 * w[k0], x1 * w[k0 + 1]};
            }
        }
    }
    constexpr int J = NC / (2 * LN);
    const int lp0 = wf_lane_part<W>(0, tid), lp1 = wf_lane_part<W>(1, tid), lp2 = wf_lane_part<W>(2, tid);
    // (a pass loads exactly the slots it stores, so one barrier per hand-over is enough)
    WfTwRaw<W, 1> raw1;
    wf_fetch_pass_tw<W, 1>(raw1, tid, twl);
    wf_apply_pass_stages<W, 0, false>(v, T0);
    wf_store<W, 0>(lds, v, lp0);
    lds_barrier();
    wf_load<W, 1>(lds, v, lp1);
    wf_unpack_pass_tw<W, 1>(T1, raw1);
    wf_apply_pass_stages<W, 1, false>(v, T1);
    WfTwRaw<W, 2> raw2;
    wf_fetch_pass_tw<W, 2>(raw2, tid, twl);
    wf_store<W, 1>(lds, v, lp1);
    lds_barrier();
    wf_load<W, 2>(lds, v, lp2);
    wf_unpack_pass_tw<W, 2>(T2, raw2);
    wf_apply_pass_stages<W, 2, false>(v, T2);
    cf sw[J];
#pragma unroll
    for (int j = 0; j < J; ++j) sw[j] = stw[tid + LN * j];
    const cf swmid = stw[NC / 2];
    wf_store<W, 2>(lds, v, lp2);
    lds_barrier();

    // real-FFT split (kiss_fftr.c:91-120): thread handles k = tid + LN j and NC - k
    const int64_t plane = ((int64_t)row * a.TR + slot);
    float *__restrict__ mag = a.mag + plane * tb.HP;
    float *__restrict__ ph = a.phase + plane * tb.HP;
    cf xlo[J], xhi[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int k = tid + LN * j;
        if (j == 0 && tid == 0) {
            const cf tdc = lds[W::pad(0)];
            xlo[0] = cf{tdc.x + tdc.y, 0.f};
            xhi[0] = cf{tdc.x - tdc.y, 0.f};
        } else {
            const cf fpk = lds[W::pad(k)];
            const cf q = lds[W::pad(NC - k)];
            const cf fpnk = cf{q.x, -q.y};
            const cf f1k = wf_add(fpk, fpnk);
            const cf f2k = wf_sub(fpk, fpnk);
            const cf tq = wf_cmul(f2k, sw[j]);
            xlo[j] = cf{(f1k.x + tq.x) * 0.5f, (f1k.y + tq.y) * 0.5f};
            xhi[j] = cf{(f1k.x - tq.x) * 0.5f, (tq.y - f1k.y) * 0.5f};
        }
    }
    cf xmid = cf{0.f, 0.f};
    if (tid == 0) {
        const cf fpk = lds[W::pad(NC / 2)];
        const cf fpnk = cf{fpk.x, -fpk.y};
        const cf f1k = wf_add(fpk, fpnk);
        const cf f2k = wf_sub(fpk, fpnk);
        const cf tq = wf_cmul(f2k, swmid);
        xmid = cf{(f1k.x - tq.x) * 0.5f, (tq.y - f1k.y) * 0.5f};
    }
    lds_barrier();
    // DC and Nyquist (zero imaginary part by construction, kiss_fftr.c:97-102: atan2f(+0, r) is +0 or pi by r's sign bit,
    // the magnitude sqrtf(r r + 0 0)) are thread 0's own values; the loop below sees (1, 1) in the DC slot, so that its
    // operand-range test is not tripped by that zero in every frame
    float dc_mag = 0.f, dc_ph = 0.f, ny_mag = 0.f, ny_ph = 0.f;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int k = tid + LN * j;
        if (j == 0 && tid == 0) {
            dc_mag = sqrtf(xlo[0].x * xlo[0].x + 0.f * 0.f);
            dc_ph = pv_u2f((uint32_t)((int32_t)pv_f2u(xlo[0].x) >> 31) & pv_f2u(3.1415927410e+00f));
            ny_mag = sqrtf(xhi[0].x * xhi[0].x + 0.f * 0.f);
            ny_ph = pv_u2f((uint32_t)((int32_t)pv_f2u(xhi[0].x) >> 31) & pv_f2u(3.1415927410e+00f));
            lds[0] = cf{1.f, 1.f};
        } else {
            lds[k] = xlo[j];
            lds[NC - k] = xhi[j];
        }
    }
    if (tid == 0) lds[NC / 2] = xmid;
    float *smag = reinterpret_cast<float *>(lds);
    *(lds_u32 *)(uintptr_t)(ATAB + 4u * (uint32_t)lane) = atab_word; // (both waves, the same words)
    lds_barrier();
    // Polar conversion, four runs of four bins per thread.  Iteration q writes its magnitudes over the cartesian values of
    // runs [64 q, 64 q + 64), which iterations 0 and 1 read -- the other wave's threads among them -- and the reads of
    // those two iterations are issued before the one barrier below; the runs of iterations 2 and 3 are never overwritten.
    constexpr int NQ = NC / (4 * LN);
    static_assert(NQ <= 4, "the hazard argument above");
    float4 nx01 = *reinterpret_cast<const float4 *>(lds + 4 * tid), nx23 = *reinterpret_cast<const float4 *>(lds + 4 * tid + 2);
    float4 nn01 = *reinterpret_cast<const float4 *>(lds + 4 * (tid + LN)), nn23 = *reinterpret_cast<const float4 *>(lds + 4 * (tid + LN) + 2);
    lds_barrier();
#pragma nounroll
    for (int q = 0; q < NQ; ++q) {
        const int i4 = 4 * (tid + LN * q);
        const float4 c01 = nx01, c23 = nx23;
        nx01 = nn01, nx23 = nn23;
        if (q + 2 < NQ) {
            nn01 = *reinterpret_cast<const float4 *>(lds + i4 + 8 * LN);
            nn23 = *reinterpret_cast<const float4 *>(lds + i4 + 8 * LN + 2);
        }
        float4 m4, p4;
        const float a0 = c01.x * c01.x + c01.y * c01.y, a1 = c01.z * c01.z + c01.w * c01.w;
        const float a2 = c23.x * c23.x + c23.y * c23.y, a3 = c23.z * c23.z + c23.w * c23.w;
        const float mx = __builtin_fmaxf(__builtin_fmaxf(pv_max3_abs(c01.x, c01.y, c01.z), pv_max3_abs(c01.w, c23.x, c23.y)),
                                         __builtin_fmaxf(__builtin_fabsf(c23.z), __builtin_fabsf(c23.w)));
        const float mn = __builtin_fminf(__builtin_fminf(pv_min3_abs(c01.x, c01.y, c01.z), pv_min3_abs(c01.w, c23.x, c23.y)),
                                         __builtin_fminf(__builtin_fabsf(c23.z), __builtin_fabsf(c23.w)));
        const bool in_range = mx < 0x1p63f && mn >= 0x1p-48f;
        if (__builtin_amdgcn_ballot_w64(!in_range) == 0) {
            m4 = make_float4(pv_sqrt_safe(a0), pv_sqrt_safe(a1), pv_sqrt_safe(a2), pv_sqrt_safe(a3));
            p4.x = pv_atan2f_fd_tab<true>(c01.y, c01.x, atab);
            p4.y = pv_atan2f_fd_tab<true>(c01.w, c01.z, atab);
            p4.z = pv_atan2f_fd_tab<true>(c23.y, c23.x, atab);
            p4.w = pv_atan2f_fd_tab<true>(c23.w, c23.z, atab);
        } else {
            m4 = make_float4(sqrtf(a0), sqrtf(a1), sqrtf(a2), sqrtf(a3));
            p4.x = pv_atan2f_fd_tab<false>(c01.y, c01.x, atab);
            p4.y = pv_atan2f_fd_tab<false>(c01.w, c01.z, atab);
            p4.z = pv_atan2f_fd_tab<false>(c23.y, c23.x, atab);
            p4.w = pv_atan2f_fd_tab<false>(c23.w, c23.z, atab);
        }
        if (q == 0 && tid == 0) p4.x = dc_ph, m4.x = dc_mag;
        *reinterpret_cast<float4 *>(ph + i4) = p4;
        *reinterpret_cast<float4 *>(mag + i4) = m4;
        *reinterpret_cast<float4 *>(smag + i4) = m4;
    }
    if (tid == 0) {
        ph[NC] = ny_ph;
        mag[NC] = ny_mag;
        smag[NC] = ny_mag; // (over cartesian bin NC / 2, which only this thread read, two iterations ago)
    }
    lds_barrier();
    if (!a.find_peaks) return; // (workgroup-uniform)
    // peak list: flags and per-wave counts first, positions once both waves' counts are known (runs in ascending bin
    // order are (q, wave 0), (q, wave 1), (q + 1, wave 0), ...)
    uint16_t *slist = reinterpret_cast<uint16_t *>(smag + NC + 4); // [PKP], 16-byte aligned
    int *scnt = reinterpret_cast<int *>(reinterpret_cast<char *>(lds) + ATAB + 4u * PV_ATAN_BLOB_WORDS); // [2][NQ] behind atan2f's table (lds is the workgroup's LDS base)
    const float inf = __builtin_inff();
    int fl[NQ], pre[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int i4 = 4 * (tid + LN * q);
        const float4 m = *reinterpret_cast<const float4 *>(smag + i4);
        float2 lo = *reinterpret_cast<const float2 *>(smag + (q == 0 && tid == 0 ? 0 : i4 - 2));
        float2 hi = *reinterpret_cast<const float2 *>(smag + i4 + 4);
        if (q == 0 && tid == 0) lo = make_float2(inf, inf);
        if (q == NQ - 1 && tid == LN - 1) hi = make_float2(inf, inf);
        const float in01 = __builtin_fmaxf(m.x, m.y), in12 = __builtin_fmaxf(m.y, m.z), in23 = __builtin_fmaxf(m.z, m.w);
        const bool f0 = m.x > __builtin_fmaxf(__builtin_fmaxf(lo.x, lo.y), in12);
        const bool f1 = m.y > __builtin_fmaxf(__builtin_fmaxf(lo.y, m.x), in23);
        const bool f2 = m.z > __builtin_fmaxf(in01, __builtin_fmaxf(m.w, hi.x));
        const bool f3 = m.w > __builtin_fmaxf(in12, __builtin_fmaxf(hi.x, hi.y));
        const bool any = f0 || f1 || f2 || f3, two = f0 && f3;
        const unsigned long long ma = __ballot(any), mb = __ballot(two);
        pre[q] = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(ma >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ma, 0u)) +
                 (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mb >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mb, 0u));
        fl[q] = (any ? 4 : 0) | (two ? 8 : 0) | (f0 ? 0 : f1 ? 1 : f2 ? 2 : 3);
        if (lane == 0) scnt[wv * NQ + q] = __popcll(ma) + __popcll(mb);
    }
    lds_barrier();
    int running = 0;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int c0 = scnt[q], c1 = scnt[NQ + q];
        const int pos = running + (wv ? c0 : 0) + pre[q];
        const int i4 = 4 * (tid + LN * q);
        if (fl[q] & 4) slist[pos] = (uint16_t)(i4 + (fl[q] & 3));
        if (fl[q] & 8) slist[pos + 1] = (uint16_t)(i4 + 3);
        running += c0 + c1;
    }
    if (tid == 0) {
        a.npk[plane] = running;
        if (running & 1) slist[running] = 0; // the odd tail shares a word with the last peak
    }
    lds_barrier();
    uint32_t *__restrict__ pk32 = reinterpret_cast<uint32_t *>(a.peaks + plane * a.PKP); // PKP % 8 == 0
    const uint32_t *slist32 = reinterpret_cast<const uint32_t *>(slist);
    for (int i = tid; 2 * i < running; i += LN) pk32[i] = slist32[i];
}

// one frame per workgroup of two waves
__global__ __launch_bounds__(128) void pv_analyze_split_kernel(const AnalyzeArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    int row, tl;
    if (!block_to_row_slice(a.Tn, a.rows, row, tl)) return; // workgroup-uniform
    analyze_split_role<WF2048S, WF2048S::LDS_CF * sizeof(cf)>(a, row, tl, reinterpret_cast<cf *>(smem_raw));
}

// (the 4096-point variant needs 232 VGPRs, two waves per SIMD; forced to three -- 168 registers, 88 spilled -- it is
// slower: 1.05 vs 0.91 ms per 64 K slices)
template <int NC, int WPB> __global__ __launch_bounds__(64 * WPB) void pv_analyze_wave_kernel(const AnalyzeArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    cf *lds = reinterpret_cast<cf *>(smem_raw) + (threadIdx.x >> 6) * WF<NC>::LDS_CF;
    int row, tl;
    if (!block_to_row_slice_w<WPB>(a.Tn, a.rows, row, tl)) return; // wave-uniform
    analyze_wave_role<NC, WPB * WF<NC>::LDS_CF * sizeof(cf)>(a, row, tl, lds);
}

// The most dynamic LDS a kernel of this file asks for (the CU's 160 KiB less a margin); every "does it fit" test and
// the attribute below use this one value.
constexpr size_t kMaxDynLds = 160 * 1024 - 512;

// Kernels may need more than the default 64 KiB of dynamic LDS.  hipFuncSetAttribute applies to the device that is
// current at the call, so the "done" mark is kept per kernel AND device (a bit per device index; atomics because two
// host threads may launch for the first time together -- setting the attribute twice is harmless).
template <typename K> static void allow_big_lds_dev(K kernel, unsigned long long &done_mask) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (__atomic_load_n(&done_mask, __ATOMIC_ACQUIRE) & bit) return;
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)kMaxDynLds);
    __atomic_fetch_or(&done_mask, bit, __ATOMIC_RELEASE);
}
// Launch of a kernel that may need the attribute: the mark lives here, one per kernel instantiation K, and the
// attribute is set before K's first launch on a device.  (Kernels that never need it are launched directly.)
template <auto K, typename... Args>
static void launch_big_lds(dim3 grid, dim3 block, size_t lds, hipStream_t st, const Args &...args) {
    static unsigned long long done_mask = 0;
    allow_big_lds_dev(K, done_mask);
    hipLaunchKernelGGL(K, grid, block, lds, st, args...);
}
// (for a launcher that chooses among instantiations of which only some need the attribute; the others fit the
// default and stay without it)
template <auto K, bool kBigLds, typename... Args>
static void launch_maybe_big_lds(dim3 grid, dim3 block, size_t lds, hipStream_t st, const Args &...args) {
    if constexpr (kBigLds) launch_big_lds<K>(grid, block, lds, st, args...);
    else hipLaunchKernelGGL(K, grid, block, lds, st, args...);
}

// (the census of the launchers' choices, below: which analysis kernel a launch is)
static void census_analysis_kernel(int set, int kernel, int nc);

void launch_analyze(const AnalyzeArgs &a, hipStream_t st) {
    const bool wave = a.tb.nc == 256 || a.tb.nc == 512 || a.tb.nc == 1024 || a.tb.nc == 2048;
    census_analysis_kernel(0, !wave ? kAnaKernelGeneric : a.tb.nc == 2048 && a.split ? kAnaKernelSplit : kAnaKernelWave, a.tb.nc);
    if (a.tb.nc == 512 || a.tb.nc == 256) { // fft 1024 / 512: four passes (pv_wavefft.h WF<512>, WF<256>)
        constexpr int WPB = 1;
        const int grid = 8 * ((a.rows + 7) / 8) * ((a.Tn + WPB - 1) / WPB);
        if (a.tb.nc == 512)
            hipLaunchKernelGGL((pv_analyze_wave_kernel<512, WPB>), dim3(grid), dim3(64 * WPB),
                               WPB * WF<512>::LDS_CF * sizeof(cf) + 4 * PV_ATAN_BLOB_WORDS, st, a);
        else
            hipLaunchKernelGGL((pv_analyze_wave_kernel<256, WPB>), dim3(grid), dim3(64 * WPB),
                               WPB * WF<256>::LDS_CF * sizeof(cf) + 4 * PV_ATAN_BLOB_WORDS, st, a);
        return;
    }
    if (a.tb.nc == 1024 || a.tb.nc == 2048) {
        if (a.tb.nc == 1024) {
            constexpr int WPB = 1; // one frame per workgroup: nothing couples the waves, and 8.6 KB of LDS each
            const int grid = 8 * ((a.rows + 7) / 8) * ((a.Tn + WPB - 1) / WPB);
            hipLaunchKernelGGL((pv_analyze_wave_kernel<1024, WPB>), dim3(grid), dim3(64 * WPB),
                               WPB * WF<1024>::LDS_CF * sizeof(cf) + 4 * PV_ATAN_BLOB_WORDS, st, a);
        } else {
            if (a.split) { // a frame on two waves (pv_analyze_split_kernel; tb.twl_fwd is WF2048S's table)
                const int grid = 8 * ((a.rows + 7) / 8) * a.Tn;
                hipLaunchKernelGGL(pv_analyze_split_kernel, dim3(grid), dim3(WF2048S::LANES),
                                   WF2048S::LDS_CF * sizeof(cf) + 4 * PV_ATAN_BLOB_WORDS + 64, st, a);
                return;
            }
            constexpr int WPB = 1;
            const int grid = 8 * ((a.rows + 7) / 8) * ((a.Tn + WPB - 1) / WPB);
            launch_big_lds<pv_analyze_wave_kernel<2048, WPB>>(dim3(grid), dim3(64 * WPB),
                               WPB * WF<2048>::LDS_CF * sizeof(cf) + 4 * PV_ATAN_BLOB_WORDS, st, a);
        }
        return;
    }
    const int grid = 8 * ((a.rows + 7) / 8) * a.Tn;
    const int nt = generic_fft_threads(a.tb.nc);
    const int J = (a.tb.hs + nt - 1) / nt;
    const size_t lds = (size_t)a.tb.nc * sizeof(float2) + sizeof(float) * (a.tb.hs + 4) + sizeof(int) * (J + 1) * 4;
    hipLaunchKernelGGL(pv_analyze_kernel, dim3(grid), dim3(nt), lds, st, a);
}

// --------------------------------------------------------------------------------------------
// phase-locked mode, parallel part: for every peak of every step, the matched previous peak and
// everything about the rotation that does not depend on the recurrence (modifySlicePhaseLocked :640-664).
// The peak lists are shared by the channels of a stream in processing order ch0, ch1, ch0, ...
// (the reference's Impl-member quirk, phasevocoderimpl.h:236-238): the "previous
// peaks" of step (t, c) are those of (t, c-1), or of (t-1, C-1) when c == 0.
// --------------------------------------------------------------------------------------------
constexpr int kMatchThreads = 256; // four waves, one step (slice) each: no workgroup barrier

// nearest set bit to position p in a bitmap of nw 64-bit words (ties -> the lower position); -1 if none
__device__ __forceinline__ int nearest_set_bit(const unsigned long long *bm, int nw, int p) {
    const int w = p >> 6, b = p & 63;
    int up = -1, dn = -1;
    unsigned long long m = bm[w] & (~0ull << b);
    for (int i = w; i < nw; ++i) {
        if (i != w) m = bm[i];
        if (m) {
            up = i * 64 + __ffsll((long long)m) - 1;
            break;
        }
    }
    m = b ? (bm[w] & ((1ull << b) - 1ull)) : 0ull;
    for (int i = w; i >= 0; --i) {
        if (i != w) m = bm[i];
        if (m) {
            dn = i * 64 + 63 - __clzll((long long)m);
            break;
        }
    }
    if (up < 0) return dn;
    if (dn < 0) return up;
    return (up - p) < (p - dn) ? up : dn;
}

// LDS bytes of one wave (= one step) of the match kernel: two bitmaps + prefix counts, then three peak lists
__host__ __device__ inline size_t match_wave_lds(int hs, int PKP) {
    const int nw = (hs + 63) >> 6;
    const size_t bm = (sizeof(unsigned long long) * 2 * nw + sizeof(int) * nw + 15) & ~(size_t)15;
    return bm + 3 * (((size_t)PKP * sizeof(uint16_t) + 15) & ~(size_t)15);
}

__device__ __forceinline__ void match_wave_role(const MatchArgs &a, const int row, const int tl, char *wbase) {
    // bitmaps instead of sorted-list searches: "nearest previous peak" is a find-first-set around p2 in the
    // previous step's peak bitmap; "region of p1" is a prefix popcount over the boundary bitmap of the previous
    // same-channel step (2-4 independent LDS reads instead of two 9-step dependent binary searches).
    // The wave's life is a chain of memory round trips, so there are three of them and no more: (1) the three
    // peak counts and, speculatively and 16 bytes per lane, the three peak lists it may need; (2) the phases at
    // the matched bins of up to six peaks per lane at once; (3) the records out.
    const int nw = (a.hs + 63) >> 6;
    unsigned long long *bprev = reinterpret_cast<unsigned long long *>(wbase);    // [nw] peaks of the previous step
    unsigned long long *bbnd = bprev + nw;                                        // [nw] region boundaries, same channel
    int *pre = reinterpret_cast<int *>(bbnd + nw);                                // [nw] boundaries before each word
    const size_t lpitch = ((size_t)a.PKP * sizeof(uint16_t) + 15) & ~(size_t)15;
    char *lbase = wbase + ((sizeof(unsigned long long) * 2 * nw + sizeof(int) * nw + 15) & ~(size_t)15);
    uint16_t *lcur = reinterpret_cast<uint16_t *>(lbase);                         // [PKP] this step's peaks
    uint16_t *lprev = reinterpret_cast<uint16_t *>(lbase + lpitch);               // [PKP] previous step's peaks
    uint16_t *lsame = reinterpret_cast<uint16_t *>(lbase + 2 * lpitch);           // [PKP] previous same-channel step's
    const int nt = 64, tid = threadIdx.x & 63;
    const int s = row / a.C, c = row - s * a.C;
    const int64_t t = a.t0 + tl;
    const int slot = ring_slot(a.s0, tl, a.TR), pslot = ring_prev(slot, a.TR);
    const int64_t plane = (int64_t)row * a.TR + slot;
    int64_t pplane = -1; // plane of the previous step
    if (c > 0) pplane = (int64_t)(row - 1) * a.TR + slot;
    else if (t > 0) pplane = (int64_t)(s * a.C + a.C - 1) * a.TR + pslot;
    const int64_t splane = t > 0 ? (int64_t)row * a.TR + pslot : -1;
    // round trip 1
    const int ncur = a.npk[plane];
    const int nprev = pplane >= 0 ? a.npk[pplane] : 0;
    const int nsame = splane >= 0 ? a.npk[splane] : 0;
    {
        const uint4 *gcur = reinterpret_cast<const uint4 *>(a.peaks + plane * a.PKP);
        const uint4 *gprev = reinterpret_cast<const uint4 *>(a.peaks + (pplane >= 0 ? pplane : plane) * a.PKP);
        const uint4 *gsame = reinterpret_cast<const uint4 *>(a.peaks + (splane >= 0 ? splane : plane) * a.PKP);
        const int n16 = a.PKP >> 3; // 16-byte pieces per list (PKP % 8 == 0)
        for (int i = tid; i < n16; i += nt) {
            const uint4 v0 = gcur[i], v1 = gprev[i], v2 = gsame[i];
            reinterpret_cast<uint4 *>(lcur)[i] = v0;
            reinterpret_cast<uint4 *>(lprev)[i] = v1;
            reinterpret_cast<uint4 *>(lsame)[i] = v2;
        }
    }
    const bool first = (t == 0 && c == 0);
    const int mode = first ? kModeInit : ((ncur == 0 || nprev == 0) ? kModeProp : kModeLock);
    if (tid == 0) {
        a.modes[plane] = mode;
        // step header in the (always free) last record slot: the sequential kernel fetches it with a vector
        // load together with its peak record, one step ahead
        PeakRec hdr{};
        hdr.p1r1 = (uint32_t)mode | ((uint32_t)ncur << 2);
        a.recs[plane * a.PKP + a.PKP - 1] = hdr;
    }
    if (mode != kModeLock) return;
    for (int i = tid; i < 2 * nw; i += nt) bprev[i] = 0ull; // bprev and bbnd are adjacent
    wave_sync();
    unsigned int *bprev32 = reinterpret_cast<unsigned int *>(bprev), *bbnd32 = reinterpret_cast<unsigned int *>(bbnd);
    for (int i = tid; i < nprev; i += nt) {
        const int b = lprev[i];
        atomicOr(&bprev32[b >> 5], 1u << (b & 31));
    }
    for (int i = tid; i + 1 < nsame; i += nt) {
        const int b = ((int)lsame[i] + (int)lsame[i + 1] + 1) >> 1;
        atomicOr(&bbnd32[b >> 5], 1u << (b & 31));
    }
    wave_sync();
    if (tid < nw) {
        int acc = 0;
        for (int i = 0; i < tid; ++i) acc += __popcll(bbnd[i]);
        pre[tid] = acc;
    }
    wave_sync();
    const float *__restrict__ A2 = a.phase + plane * a.HP;
    const float *__restrict__ A1 = a.phase + (splane >= 0 ? splane : plane) * a.HP;
    const float pinc_f = (float)a.phase_inc[tl], hop_f = (float)a.hop;
    const double Nd = (double)a.N;
    constexpr int kU = 6; // peaks per lane whose phase gathers are in flight together (hs 1024: all of them)
    for (int pb = 0; pb < ncur; pb += nt * kU) {
        int p2v[kU], p1v[kU];
        float a2v[kU], a1v[kU];
        // round trip 2
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int p = pb + tid + nt * u;
            p2v[u] = lcur[p < ncur ? p : ncur - 1];
            // nearest previous peak, ties -> lower bin (== the reference's monotone greedy walk :644-652)
            p1v[u] = nearest_set_bit(bprev, nw, p2v[u]);
            a2v[u] = A2[p2v[u]];
            a1v[u] = A1[p1v[u]]; // prev_phase of this channel == its previous analysis phase
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int p = pb + tid + nt * u;
            if (p >= ncur) continue;
            const int p2 = p2v[u], p1 = p1v[u];
            const float avg_p = (float)((double)(p1 + p2) * 0.5);
            const float pomega = (float)((a.two_pi_hop * (double)(avg_p - 1)) / Nd);
            const float a2 = a2v[u];
            const float a1 = splane >= 0 ? a1v[u] : 0.f;
            const float d1 = a2 - a1 - pomega;
            const float pdelta = (float)((double)pomega + princarg_f(d1));
            // region of p1 in the previous same-channel step = number of its boundaries <= p1
            const int w1 = p1 >> 6, b1 = p1 & 63;
            const unsigned long long le = b1 == 63 ? ~0ull : ((2ull << b1) - 1ull);
            const int r1 = pre[w1] + __popcll(bbnd[w1] & le);
            PeakRec r;
            r.adv = (pdelta * pinc_f) / hop_f;
            r.a2 = a2;
            r.a1 = a1;
            r.p1r1 = (uint32_t)p1 | ((uint32_t)r1 << 16);
            a.recs[plane * a.PKP + p] = r; // round trip 3
        }
    }
}

__global__ __launch_bounds__(kMatchThreads) void pv_match_kernel(const MatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    const int wave = threadIdx.x >> 6;
    const int tl = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave);
    if (tl >= a.Tn) return; // wave-uniform
    match_wave_role(a, blockIdx.y, tl, smem_raw + (size_t)wave * match_wave_lds(a.hs, a.PKP));
}

void launch_match(const MatchArgs &a, hipStream_t st) {
    const size_t lds = 4 * match_wave_lds(a.hs, a.PKP);
    hipLaunchKernelGGL(pv_match_kernel, dim3((a.Tn + 3) / 4, a.rows), dim3(kMatchThreads), lds, st, a);
}

// --------------------------------------------------------------------------------------------
// phase-locked mode, sequential part: one workgroup per (stream, channel) row walks its slices in
// order.  In a LOCK step only the peaks carry the recurrence:
//   target = princarg(prev_out[p1] + adv),  rot = princarg(target - phase[p2])         (:664-665)
// and prev_out[p1] of a locked previous step is princarg(prev_phase[p1] + rot_prev[region(p1)]) (:688,697),
// evaluated lazily here.  Every other bin's output phase is applied later, in parallel, by the
// synthesis kernel.  INIT / PROP steps (first slice, silence: no peaks) take the per-bin path (:606-636).
// --------------------------------------------------------------------------------------------
__device__ __forceinline__ int region_of(const uint16_t *pk, int n, int i) {
    // number of boundaries round((pk[j] + pk[j+1]) / 2) (half away from zero, :676-682) that are <= i
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int bnd = ((int)pk[mid] + (int)pk[mid + 1] + 1) >> 1;
        if (bnd <= i) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// kK: peaks per lane in the fast loop (1: a lane per peak, six waves per row at 2048 points; 3: two waves per row --
// a third of the wave slots and registers beside whatever shares the CU, at the price of a longer step)
template <int kK = 1>
__device__ __forceinline__ void seq_role(const SeqArgs &a, const int row, char *smem_raw) {
    float *srot0 = reinterpret_cast<float *>(smem_raw);          // [PKP]
    float *srot1 = srot0 + a.PKP;                                // [PKP]
    float *spo = srot1 + a.PKP;                                  // [hs] full prev_out (valid when kind == 1)
    uint16_t *spk = reinterpret_cast<uint16_t *>(spo + a.hs);    // [PKP] peaks of the previous same-row step
    const int nt = blockDim.x, tid = threadIdx.x, hs = a.hs;
    const int c = row % a.C;
    int kind = a.st_kind[row];
    float *rprev = srot0, *rcur = srot1;
    if (kind == 2)
        for (int i = tid; i < a.PKP; i += nt) rprev[i] = a.st_rot[(int64_t)row * a.PKP + i];
    if (kind == 1)
        for (int i = tid; i < hs; i += nt) spo[i] = a.st_po[(int64_t)row * hs + i];
    __syncthreads();
    const float hop_f = (float)a.hop;
    const double Nd = (double)a.N;

    // the step's inputs (mode, peak count, this lane's peak record) do not depend on the recurrence: they are
    // fetched one step ahead so the global-load latency overlaps the previous step's princarg chain
    const bool one_pass = a.PKP <= kK * nt; // every peak has its own lane (or one of a lane's kK slots)
    auto plane_of = [&](int tl) { return (int64_t)row * a.TR + ring_slot(a.s0, tl, a.TR); };
    // (one_pass: every peak has its own lane)
    // The header is wave-uniform, but it must come through the vector memory path: a scalar load shares its
    // counter (lgkmcnt) with the LDS reads of the chain and would put its latency back on the critical path.
    // An opaque zero in a VGPR keeps the compiler from scalarising the address.
    int vz = 0;
    asm volatile("" : "+v"(vz));
    // unconditional (index clamped): a load inside an exec-masked branch gets its s_waitcnt at the end of
    // the branch, which would defeat the prefetch
    int rixk[kK];
#pragma unroll
    for (int k = 0; k < kK; ++k) rixk[k] = tid + k * nt < a.PKP ? tid + k * nt : a.PKP - 1;
    const int rix = rixk[0];
    // Prefetch ONE step ahead.  Measured alternatives (all slower alone on the GPU): queues 4 and 6 steps deep
    // (+15 %: the chain, not the load latency, bounds a step), always-clamped loads instead of the uniform
    // last-step branch (+13 %).
    auto ld_hdr = [&](int tl) -> uint32_t { return a.recs[plane_of(tl) * a.PKP + a.PKP - 1 + vz].p1r1; };
    auto ld_rec = [&](int tl) -> PeakRec { return a.recs[plane_of(tl) * a.PKP + rix]; };
    auto ld_recs = [&](int tl, PeakRec (&q)[kK]) {
#pragma unroll
        for (int k = 0; k < kK; ++k) q[k] = a.recs[plane_of(tl) * a.PKP + rixk[k]];
    };
    uint32_t h0 = ld_hdr(0);
    PeakRec qk[kK];
    ld_recs(0, qk);
    (void)ld_rec;

    int tl = 0;
    while (tl < a.Tn) {
        // ---- fast inner loop: consecutive phase-locked steps.  It contains exactly two prefetch loads followed
        // by one store per iteration, so the loop-top wait can be the counted vmcnt(1) (the store stays in
        // flight); the slow per-bin path lives outside this loop precisely to keep that count static.
        while (tl < a.Tn && (h0 & 3u) == (uint32_t)kModeLock && one_pass) {
            const int64_t plane = plane_of(tl);
            PeakRec rk[kK];
#pragma unroll
            for (int k = 0; k < kK; ++k) rk[k] = qk[k];
            if (tl + 1 < a.Tn) { // uniform branch
#if !(defined(PV_EXP_SEQ) && (PV_EXP_SEQ & 16))
                h0 = ld_hdr(tl + 1);
                ld_recs(tl + 1, qk);
#endif
            } else {
                h0 = 3u; // sentinel: leaves both loops
            }
            // Branch-free over the lanes: lanes beyond the peak count run on whatever their (clamped) record
            // slot holds and write slots nobody reads.
            // straight-line code (princarg_div has no rare-case branch): any branch inside this loop makes the
            // compiler fall back to vmcnt(0) at the joins, which exposes the store latency under load
            float rtk[kK];
#pragma unroll
            for (int k = 0; k < kK; ++k) {
                const PeakRec r = rk[k];
                const uint32_t r1 = min(r.p1r1 >> 16, (uint32_t)(a.PKP - 1));
                const uint32_t p1 = (r.p1r1 & 0xffffu) & (uint32_t)(hs - 1);
                // (PV_EXP_SEQ: elimination builds for timing only -- tools/build_variant.sh, tools/seq_elim.sh -- bit 0 no
                // princarg_small, 1 no princarg_f, 2 no global store, 3 no barrier, 4 no record prefetch)
#if defined(PV_EXP_SEQ) && (PV_EXP_SEQ & 1)
                const float po_lock = r.a1 + rprev[r1];
#else
                const float po_lock = (float)princarg_small((double)(r.a1 + rprev[r1]));
#endif
                const float po_full = spo[p1];
                const float po = kind == 2 ? po_lock : (kind == 1 ? po_full : 0.f);
#if defined(PV_EXP_SEQ) && (PV_EXP_SEQ & 2)
                const float tgt = po + r.adv;
#else
                const float tgt = (float)princarg_f(po + r.adv);
#endif
#if defined(PV_EXP_SEQ) && (PV_EXP_SEQ & 1)
                rtk[k] = tgt - r.a2;
#else
                rtk[k] = (float)princarg_small((double)(tgt - r.a2));
#endif
            }
#pragma unroll
            for (int k = 0; k < kK; ++k) {
                rcur[rixk[k]] = rtk[k];
#if !(defined(PV_EXP_SEQ) && (PV_EXP_SEQ & 4))
                a.rot[plane * a.PKP + rixk[k]] = rtk[k];
#endif
            }
            kind = 2;
            float *tmp = rprev;
            rprev = rcur;
            rcur = tmp;
            ++tl;
#if defined(PV_EXP_SEQ) && (PV_EXP_SEQ & 8)
            __builtin_amdgcn_s_waitcnt(0xc07f); // lgkmcnt(0) only: no barrier (timing experiment)
#else
            __syncthreads();
#endif
        }
        if (tl >= a.Tn) break;
        // ---- general step (first slice, no-peak steps, or more peaks than lanes)
        const int64_t t = a.t0 + tl;
        const int64_t plane = plane_of(tl);
        const int mode = (int)(h0 & 3u), n = (int)(h0 >> 2);
        if (tl + 1 < a.Tn) {
            h0 = ld_hdr(tl + 1);
            ld_recs(tl + 1, qk);
        }
        if (mode == kModeLock) {
            for (int p = tid; p < n; p += nt) {
                const PeakRec r = a.recs[plane * a.PKP + p];
                float po;
                if (kind == 2) po = (float)princarg_small((double)(r.a1 + rprev[r.p1r1 >> 16]));
                else if (kind == 1) po = spo[r.p1r1 & 0xffffu];
                else po = 0.f;
                const float tgt = (float)princarg_f(po + r.adv);
                const float rt = (float)princarg_small((double)(tgt - r.a2));
                rcur[p] = rt;
                a.rot[plane * a.PKP + p] = rt;
            }
            kind = 2;
            float *tmp = rprev;
            rprev = rcur;
            rcur = tmp;
        } else {
            // per-bin path; first materialise prev_out when the previous step of this row was locked
            const float *__restrict__ A = a.phase + plane * a.HP;
            const int64_t splane = t > 0 ? (int64_t)row * a.TR + ring_prev(ring_slot(a.s0, tl, a.TR), a.TR) : -1;
            const float *__restrict__ Ap = splane >= 0 ? a.phase + splane * a.HP : nullptr;
            int nsame = 0;
            if (kind == 2) {
                nsame = a.npk[splane];
                for (int i = tid; i < nsame; i += nt) spk[i] = a.peaks[splane * a.PKP + i];
                __syncthreads();
            }
            const float pinc_f = (float)a.phase_inc[tl];
            float *__restrict__ outp = a.outphase + plane * a.HP;
            for (int i = tid; i < hs; i += nt) {
                const float phi = A[i];
                float outv;
                if (mode == kModeInit) {
                    outv = phi;
                } else {
                    float po;
                    if (kind == 2) po = (float)princarg_small((double)(Ap[i] + rprev[region_of(spk, nsame, i)]));
                    else if (kind == 1) po = spo[i];
                    else po = 0.f;
                    const float pp = Ap ? Ap[i] : 0.f;
                    const float omega = (float)((a.two_pi_hop * (double)i) / Nd);
                    const float d1 = phi - pp - omega;
                    const float delta = (float)((double)omega + princarg_f(d1));
                    const float advance = delta * pinc_f / hop_f;
                    outv = (float)princarg_f(po + advance);
                }
                spo[i] = outv;
                outp[i] = outv;
            }
            kind = 1;
        }
        ++tl;
        __syncthreads();
    }
    if (kind == 2)
        for (int i = tid; i < a.PKP; i += nt) a.st_rot[(int64_t)row * a.PKP + i] = rprev[i];
    if (kind == 1)
        for (int i = tid; i < hs; i += nt) a.st_po[(int64_t)row * hs + i] = spo[i];
    if (tid == 0) a.st_kind[row] = kind;
    (void)c;
}

__host__ __device__ size_t seq_lds_bytes(const SeqArgs &a);
// --------------------------------------------------------------------------------------------
// The same walk with the step records prefetched kSeqDepth steps ahead through an LDS ring (round 3).  Elimination
// builds (profiles/r02/seq_elim.txt) showed that a step of the loop above IS the latency of its one-step-ahead record
// load (0.94 us with it, 0.54 without); register queues four to eight steps deep lost to the compiler's waits and
// spills.  Here a wave fetches its own 64 records of step t + kSeqDepth - 1 with ONE global_load_lds_dwordx4 (LDS-DMA:
// no destination registers, so nothing to spill and nothing the compiler waits for) into slot (t - 1) % kSeqDepth --
// the slot step t - 1 has just finished with -- and reads step t's records from LDS.  The loads, the rotation store
// and their waits are inline assembly so that the vmcnt counts below are exact; the compiler sees no vector memory
// operation in the fast loop.  Arithmetic: the loop above, operation for operation.
//
// Waits.  VM operations retire in issue order (one counter on gfx9).  At the end of iteration t the records of step
// t + 1 must have landed.  Issued behind that load by then: the loads of steps t + 2 .. t + kSeqDepth - 1 (those that
// exist) and one store per iteration since it was issued, so
//     steady state (the last kSeqDepth - 1 iterations all took the fast path):  vmcnt(2 kSeqDepth - 3)
//     conservative (start of the launch, behind a general step):               vmcnt(kSeqDepth - 2), loads only
//     tail (no more loads issued):                                             vmcnt(kSeqDepth - 1) resp. vmcnt(0)
// a count that is too small only waits longer.  The wait sits in front of the step's barrier, the read behind it: the
// step header (last record slot) is read by every wave, and data an LDS-DMA wrote is another wave's to read only
// after that wave's wait and a barrier.
// --------------------------------------------------------------------------------------------
constexpr int kSeqDepthMax = 8;

__device__ __forceinline__ void seq_glds16(const void *gsrc, uint32_t lds_dst) { // lds_dst: wave-uniform byte address
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gsrc), "s"(lds_dst)
                 : "memory");
}
template <int N> __device__ __forceinline__ void seq_wait_barrier() {
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(N < 0 ? 0 : N) : "memory");
}

// (the step's own LDS reads -- header and record -- are issued one step ahead as well, at the top of the step before,
// so that a step's dependent chain is what it was with the record in registers: rotation read, three wraps, rotation
// write, barrier.  Hence the waits below are for step t + 2.)
template <int D> __device__ __forceinline__ void seq_role_ring(const SeqArgs &a, const int row, char *smem_raw) {
    static_assert(D >= 4 && D <= kSeqDepthMax, "ring depth");
    float *srot0 = reinterpret_cast<float *>(smem_raw);          // [PKP]
    float *srot1 = srot0 + a.PKP;                                // [PKP]
    float *spo = srot1 + a.PKP;                                  // [hs] full prev_out (valid when kind == 1)
    uint16_t *spk = reinterpret_cast<uint16_t *>(spo + a.hs);    // [PKP] peaks of the previous same-row step
    const int nt = blockDim.x, tid = threadIdx.x, hs = a.hs;
    PeakRec *ring = reinterpret_cast<PeakRec *>(smem_raw + ((seq_lds_bytes(a) + 15) & ~(size_t)15)); // [D][nt]
    const uint32_t ring_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char *)reinterpret_cast<char *>(ring);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int kind = a.st_kind[row];
    float *rprev = srot0, *rcur = srot1;
    if (kind == 2)
        for (int i = tid; i < a.PKP; i += nt) rprev[i] = a.st_rot[(int64_t)row * a.PKP + i];
    if (kind == 1)
        for (int i = tid; i < hs; i += nt) spo[i] = a.st_po[(int64_t)row * hs + i];
    __syncthreads(); // (the compiler's loads above are complete: it waited for their values)
    const float hop_f = (float)a.hop;
    const double Nd = (double)a.N;
    auto plane_of = [&](int tl) { return (int64_t)row * a.TR + ring_slot(a.s0, tl, a.TR); };
    const int rix = tid < a.PKP ? tid : a.PKP - 1; // (nt >= PKP: every peak has its own lane)
    auto fetch = [&](int step) { // this wave's 64 records of `step` into the step's ring slot
        const PeakRec *src = a.recs + plane_of(step) * a.PKP + rix;
        const uint32_t dst = ring_lds + (uint32_t)(((step % D) * nt + wave * 64) * (int)sizeof(PeakRec));
        seq_glds16(src, __builtin_amdgcn_readfirstlane(dst));
    };
    for (int sft = 0; sft < D - 1 && sft < a.Tn; ++sft) fetch(sft);
    if (a.Tn >= D - 1) seq_wait_barrier<D - 3>(); // steps 0 and 1 have landed (D - 3 younger loads may be in flight)
    else seq_wait_barrier<0>();
    uint32_t h_next = ring[a.PKP - 1].p1r1;
    PeakRec r_next = ring[tid];

    int fast_run = 0; // consecutive iterations, ending with the current one, that issued exactly one (asm) store
    for (int tl = 0; tl < a.Tn; ++tl) {
        if (tl - 1 + D < a.Tn) fetch(tl - 1 + D); // into the slot step tl - 1 used: every wave is past that step's barrier
        const uint32_t h0 = h_next;
        const PeakRec r = r_next;
        if (tl + 1 < a.Tn) { // the next step's header and record (landed: the wait at the end of step tl - 1)
            const PeakRec *slot = ring + ((tl + 1) % D) * nt;
            h_next = slot[a.PKP - 1].p1r1;
            r_next = slot[tid];
        }
        const int mode = (int)(h0 & 3u);
        const int64_t plane = plane_of(tl);
        if (mode == kModeLock) {
            // ---- phase-locked step: branch-free over the lanes (lanes beyond the peak count run on whatever their
            // record slot holds and write slots nobody reads)
            const uint32_t r1 = min(r.p1r1 >> 16, (uint32_t)(a.PKP - 1));
            const uint32_t p1 = (r.p1r1 & 0xffffu) & (uint32_t)(hs - 1);
            const float po_lock = (float)princarg_small((double)(r.a1 + rprev[r1]));
            const float po_full = spo[p1];
            const float po = kind == 2 ? po_lock : (kind == 1 ? po_full : 0.f);
            const float tgt = (float)princarg_f(po + r.adv);
            const float rt = (float)princarg_small((double)(tgt - r.a2));
            rcur[rix] = rt;
            {
                float *dst = a.rot + plane * a.PKP + rix;
                asm volatile("global_store_dword %0, %1, off" ::"v"(dst), "v"(rt) : "memory");
            }
            kind = 2;
            float *tmp = rprev;
            rprev = rcur;
            rcur = tmp;
            ++fast_run;
        } else {
            // ---- per-bin step (first slice, silence): prev_out materialised when the previous step was locked
            fast_run = 0;
            const int64_t t = a.t0 + tl;
            const float *__restrict__ A = a.phase + plane * a.HP;
            const int64_t splane = t > 0 ? (int64_t)row * a.TR + ring_prev(ring_slot(a.s0, tl, a.TR), a.TR) : -1;
            const float *__restrict__ Ap = splane >= 0 ? a.phase + splane * a.HP : nullptr;
            int nsame = 0;
            if (kind == 2) {
                nsame = a.npk[splane];
                for (int i = tid; i < nsame; i += nt) spk[i] = a.peaks[splane * a.PKP + i];
                __syncthreads();
            }
            const float pinc_f = (float)a.phase_inc[tl];
            float *__restrict__ outp = a.outphase + plane * a.HP;
            for (int i = tid; i < hs; i += nt) {
                const float phi = A[i];
                float outv;
                if (mode == kModeInit) {
                    outv = phi;
                } else {
                    float po;
                    if (kind == 2) po = (float)princarg_small((double)(Ap[i] + rprev[region_of(spk, nsame, i)]));
                    else if (kind == 1) po = spo[i];
                    else po = 0.f;
                    const float pp = Ap ? Ap[i] : 0.f;
                    const float omega = (float)((a.two_pi_hop * (double)i) / Nd);
                    const float d1 = phi - pp - omega;
                    const float delta = (float)((double)omega + princarg_f(d1));
                    const float advance = delta * pinc_f / hop_f;
                    outv = (float)princarg_f(po + advance);
                }
                spo[i] = outv;
                outp[i] = outv;
            }
            kind = 1;
        }
        // ---- the records of step tl + 2 have landed; then the step's barrier
        if (tl + 2 >= a.Tn) {
            seq_wait_barrier<0>();
        } else if (fast_run >= D - 2) {
            if (tl - 1 + D < a.Tn) seq_wait_barrier<2 * D - 5>();
            else seq_wait_barrier<D - 2>();
        } else {
            if (tl - 1 + D < a.Tn) seq_wait_barrier<D - 3>();
            else seq_wait_barrier<0>();
        }
    }
    if (kind == 2)
        for (int i = tid; i < a.PKP; i += nt) a.st_rot[(int64_t)row * a.PKP + i] = rprev[i];
    if (kind == 1)
        for (int i = tid; i < hs; i += nt) a.st_po[(int64_t)row * hs + i] = spo[i];
    if (tid == 0) a.st_kind[row] = kind;
}

template <int D> __global__ __launch_bounds__(1024) void pv_seq_ring_kernel(const SeqArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    if (a.high_prio) __builtin_amdgcn_s_setprio(3);
    seq_role_ring<D>(a, blockIdx.x, smem_raw);
}

template <int kK> __global__ __launch_bounds__(1024) void pv_seq_kernel(const SeqArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    // the chain is pure latency and may share the GPU with the overlap-add tiles of the previous chunk (second
    // HIP stream): let its few waves win every issue arbitration
    if (a.high_prio) __builtin_amdgcn_s_setprio(3);
    seq_role<kK>(a, blockIdx.x, smem_raw);
}

// Single-stream engine: match and rotation chain in ONE launch (round 3).  A 480-frame call is two or three steps per
// row: far too little for the two kernels to need separate grids, and every launch costs the host ~7 us of the call's
// ~70.  One workgroup per row: its waves match the row's steps (a step's match depends on analysis results only, of
// this row and its neighbour channel -- nothing another workgroup of this launch writes), then, behind a device-scope
// fence and a barrier, the same workgroup walks the chain.  Same device functions, same results.
template <int D> __global__ __launch_bounds__(1024) void pv_phase_kernel(const MatchArgs m, const SeqArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
    for (int tl = wave; tl < m.Tn; tl += nw)
        match_wave_role(m, blockIdx.x, tl, smem_raw + (size_t)wave * match_wave_lds(m.hs, m.PKP));
    __threadfence(); // the records go through global memory: the chain's loads must see them
    __syncthreads();
    if (a.high_prio) __builtin_amdgcn_s_setprio(3);
    seq_role_ring<D>(a, blockIdx.x, smem_raw);
}

int seq_threads(int PKP) {
    int nt = (PKP + 63) & ~63;
    if (nt > 1024) nt = 1024;
    if (nt < 64) nt = 64;
    return nt;
}
__host__ __device__ size_t seq_lds_bytes(const SeqArgs &a) { return sizeof(float) * ((size_t)2 * a.PKP + a.hs) + sizeof(uint16_t) * a.PKP; }

// (the census of the launchers' choices, below: a = form, b = ring depth or peaks per lane)
static void census_phase(int set, int form, int b);

void launch_seq(const SeqArgs &a, hipStream_t st) {
    const size_t lds = seq_lds_bytes(a);
    if (a.narrow && a.PKP <= 3 * 1024) {
        // three peaks per lane: a third of the waves (two per row at 2048 points), so that the kernel finds room on
        // a CU beside the fused kernel's workgroup
        int nt = ((a.PKP + 2) / 3 + 63) & ~63;
        if (nt > 1024) nt = 1024;
        census_phase(0, kPhaseFormStep, 3);
        launch_big_lds<pv_seq_kernel<3>>(dim3(a.rows), dim3(nt), lds, st, a);
        return;
    }
    const int nt = seq_threads(a.PKP);
    static const bool no_ring = [] { // AUDIOMOD_PV_SEQ_RING=0: round 2's one-step-ahead register prefetch (for A/B runs)
        const char *e = getenv("AUDIOMOD_PV_SEQ_RING");
        return e && atoi(e) == 0;
    }();
    static const int depth = [] { // AUDIOMOD_PV_SEQ_DEPTH=4|8 (tuning knob)
        const char *e = getenv("AUDIOMOD_PV_SEQ_DEPTH");
        return e ? atoi(e) : 0;
    }();
    // Four steps ahead where the kernel shares its CUs with a full batch's other kernels (a deeper ring's LDS then
    // costs more than its latency cover returns: 0.58 vs 0.38 ms per launch beside the resampling kernel); eight for
    // small batches, which are bound by this chain and leave the LDS free (20 streams: 10.6 -> 11.0 G samples/s).
    const int D = depth ? (depth <= 4 ? 4 : 8) : (a.rows <= 96 ? 8 : 4);
    const size_t ring_lds = ((lds + 15) & ~(size_t)15) + (size_t)D * nt * sizeof(PeakRec);
    if (!no_ring && a.PKP <= nt && ring_lds <= kMaxDynLds) {
        census_phase(0, kPhaseFormRing, D);
        if (D == 4) {
            launch_big_lds<pv_seq_ring_kernel<4>>(dim3(a.rows), dim3(nt), ring_lds, st, a);
        } else {
            launch_big_lds<pv_seq_ring_kernel<8>>(dim3(a.rows), dim3(nt), ring_lds, st, a);
        }
        return;
    }
    census_phase(0, kPhaseFormStep, 1);
    launch_big_lds<pv_seq_kernel<1>>(dim3(a.rows), dim3(nt), lds, st, a);
}

// (true when the fused kernel was launched; false: the caller launches the two kernels)
bool launch_phase(const MatchArgs &m, const SeqArgs &a, hipStream_t st) {
    constexpr int D = 8;
    const int nt = seq_threads(a.PKP);
    const size_t seq_l = ((seq_lds_bytes(a) + 15) & ~(size_t)15) + (size_t)D * nt * sizeof(PeakRec);
    const size_t match_l = (size_t)(nt / 64) * match_wave_lds(m.hs, m.PKP);
    const size_t lds = seq_l > match_l ? seq_l : match_l;
    if (a.PKP > nt || lds > kMaxDynLds || a.narrow) return false;
    census_phase(0, kPhaseFormFused, D);
    launch_big_lds<pv_phase_kernel<D>>(dim3(a.rows), dim3(nt), lds, st, m, a);
    return true;
}

// --------------------------------------------------------------------------------------------
// coremode 0 (modifySliceSimple :708-753): independent per-bin recurrences; one thread per bin streams
// over the slices of the launch with its state in registers.
// --------------------------------------------------------------------------------------------
constexpr int kPropThreads = 256;

__device__ __forceinline__ void prop_role(const PropArgs &a, const int row, const int i) {
    // Only out = princarg(prev_out + advance) is a recurrence: the advance of a step depends on the analysis phases
    // of that step and the one before, which are data.  So the slices are taken four at a time -- their phases
    // loaded together, their advances computed side by side -- and only the last princarg of each forms the chain.
    const int c = row % a.C;
    const float *__restrict__ ph = a.phase;
    float *__restrict__ op = a.outphase;
    float pp = a.st_pp[(int64_t)row * a.hs + i], po = a.st_po[(int64_t)row * a.hs + i];
    const float omega = (float)((a.two_pi_hop * (double)i) / (double)a.N);
    const float hop_f = (float)a.hop;
    constexpr int kU = 4;
    for (int tl0 = 0; tl0 < a.Tn; tl0 += kU) {
        float phi[kU], adv[kU];
        int64_t plane[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int tl = tl0 + u < a.Tn ? tl0 + u : a.Tn - 1;
            plane[u] = (int64_t)row * a.TR + ring_slot(a.s0, tl, a.TR);
            phi[u] = ph[plane[u] * a.HP + i];
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int tl = tl0 + u < a.Tn ? tl0 + u : a.Tn - 1;
            const float d1 = phi[u] - (u ? phi[u - 1] : pp) - omega;
            const float delta = (float)((double)omega + princarg_f(d1));
            adv[u] = delta * (float)a.phase_inc[tl] / hop_f;
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            if (tl0 + u >= a.Tn) break;
            // firstentry: only the very first step of the stream (function-static in the reference)
            const float outv = (a.t0 + tl0 + u == 0 && c == 0) ? phi[u] : (float)princarg_f(po + adv[u]);
            pp = phi[u];
            po = outv;
            op[plane[u] * a.HP + i] = outv;
        }
    }
    a.st_pp[(int64_t)row * a.hs + i] = pp;
    a.st_po[(int64_t)row * a.hs + i] = po;
}

__global__ __launch_bounds__(kPropThreads) void pv_prop_kernel(const PropArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.hs) prop_role(a, blockIdx.y, i);
}

void launch_prop(const PropArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(pv_prop_kernel, dim3((a.hs + kPropThreads - 1) / kPropThreads, a.rows), dim3(kPropThreads), 0,
                       st, a);
}

// --------------------------------------------------------------------------------------------
// synthesis (+ per-bin application of the phase modification)
// --------------------------------------------------------------------------------------------
// modifySliceVocoder (phasevocoderprocess.cc:755-776): carrier magnitude of bin k times the mean modulator
// magnitude of its band (band_len bins, float running sum from 0, divided by band_len*2); DC and Nyquist zeroed.
__device__ __forceinline__ float vocoder_mag(const float *__restrict__ mod, const float *__restrict__ cmag, int k,
                                             int hs, int band_len) {
    if (k == 0 || k == hs) return 0.f;
    float mg = cmag[k];
    if (band_len > 0 && k < 512 * band_len) {
        const int j0 = (k / band_len) * band_len;
        float mean = 0.f;
        for (int i = 0; i < band_len; ++i) mean += mod[j0 + i];
        mean /= (float)(band_len * 2);
        mg *= mean;
    }
    return mg;
}

__global__ __launch_bounds__(kFftThreads) void pv_synth_kernel(const SynthArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    const DevTables &tb = a.tb;
    const int N = tb.N, hs = tb.hs, nc = tb.nc, nt = blockDim.x;
    float2 *buf = reinterpret_cast<float2 *>(smem_raw);        // [nc]
    float2 *X = buf + nc;                                      // [nc + 1]
    float *sph = reinterpret_cast<float *>(X + nc + 1);        // [hs + 1] output phase of every bin
    float *srot = sph + hs + 4;                                // [PKP]
    uint16_t *spk = reinterpret_cast<uint16_t *>(srot + a.PKP); // [PKP]
    int row, tl;
    if (!block_to_row_slice(a.Tn, a.rows, row, tl)) return;
    const int64_t t = a.t0 + tl;
    const int64_t plane = (int64_t)row * a.TR + ring_slot(a.s0, tl, a.TR);
    const float *__restrict__ mag = a.mag + plane * tb.HP;
    const float *__restrict__ A = a.phase + plane * tb.HP;
    const double Nd = (double)N;

    // 1. output phase of every bin
    const int cslot = ring_slot(a.s0, tl, a.TR);
    if (a.voc_band_len >= 0) {
        const float *__restrict__ cp = a.cphase + (int64_t)cslot * tb.HP;
        for (int k = threadIdx.x; k <= hs; k += nt) sph[k] = cp[k];
    } else if (a.robotic) {
        for (int k = threadIdx.x; k <= hs; k += nt) sph[k] = 0.f;
    } else if (a.passthru) {
        for (int k = threadIdx.x; k <= hs; k += nt) sph[k] = A[k];
    } else if (a.whisper) {
        const float *__restrict__ wp = a.whisper + ((int64_t)tl * a.C + row % a.C) * tb.HP;
        for (int k = threadIdx.x; k <= hs; k += nt) sph[k] = wp[k];
    } else if (a.coremode == 2) {
        const float pinc_f = (float)a.phase_inc[tl], hop_f = (float)a.hop;
        for (int k = threadIdx.x; k <= hs; k += nt) sph[k] = k < hs ? A[k] * pinc_f / hop_f : A[k];
    } else {
        const int mode = a.coremode == 1 ? a.modes[plane] : kModeProp;
        if (mode == kModeLock) {
            const int n = a.npk[plane];
            for (int i = threadIdx.x; i < n; i += nt) {
                spk[i] = a.peaks[plane * a.PKP + i];
                srot[i] = a.rot[plane * a.PKP + i];
            }
            __syncthreads();
            for (int k = threadIdx.x; k <= hs; k += nt) {
                const float phi = A[k];
                sph[k] = k < hs ? (float)princarg_small((double)(phi + srot[region_of(spk, n, k)])) : phi;
            }
        } else {
            const float *__restrict__ op = a.outphase + plane * tb.HP;
            for (int k = threadIdx.x; k <= hs; k += nt) sph[k] = k < hs ? op[k] : A[k];
        }
    }
    __syncthreads();

    // 2. spectrum: freqCompSlice gather (:869-916, both branches are pure gathers from the pre-call arrays),
    //    gains, polar -> cartesian (FFT.cc:2711-2718)
    for (int k = threadIdx.x; k <= hs; k += nt) {
        float mg, p;
        if (a.do_freq_comp) {
            if (a.freq_comp > 1.0f) {
                const int src = __float2int_rn((float)k * a.freq_comp);
                if (src > hs) {
                    mg = 0.f;
                    p = 0.f;
                } else {
                    mg = mag[src];
                    p = sph[src] + (float)((a.two_pi_hop * (double)(k - src)) / Nd);
                }
            } else if (k < hs) {
                const int src = __float2int_rn((float)k * a.freq_comp);
                mg = mag[src];
                p = sph[src] + (float)((a.two_pi_hop * (double)(k - src)) / Nd);
            } else {
                mg = mag[k];
                p = sph[k];
            }
            mg *= a.fixed_gain;
        } else if (a.voc_band_len >= 0) {
            mg = vocoder_mag(mag, a.cmag + (int64_t)cslot * tb.HP, k, hs, a.voc_band_len);
            p = sph[k];
        } else {
            mg = mag[k];
            p = sph[k];
        }
        mg *= a.inv_n;
        X[k] = make_float2(mg * cosf(p), mg * sinf(p));
    }
    __syncthreads();

    // 3. kiss_fftri pre-pass (kiss_fftr.c:134-157), scattered straight into butterfly order
    for (int k = threadIdx.x; k <= nc / 2; k += nt) {
        if (k == 0) {
            buf[tb.iperm[0]] = make_float2(X[0].x + X[nc].x, X[0].x - X[nc].x);
        } else {
            const float2 fk = X[k];
            const float2 q = X[nc - k];
            const float2 fnkc = make_float2(q.x, -q.y);
            const float2 fek = cadd(fk, fnkc);
            const float2 tq = csub(fk, fnkc);
            const float2 fok = cmul(tq, tb.st_inv[k]);
            const float2 u = cadd(fek, fok);
            float2 v = csub(fek, fok);
            v.y = v.y * -1.f;
            if (k != nc - k) buf[tb.iperm[k]] = u;
            buf[tb.iperm[nc - k]] = v;
        }
    }
    __syncthreads();
    fft_stages<true>(buf, tb, tb.tw_inv);

    // 4. ifftshift + synthesis window (phasevocoderimpl.h:183-198)
    const float *fb = reinterpret_cast<const float *>(buf);
    const int fslot = (int)(t & (int64_t)(a.FR - 1));
    float *__restrict__ out = a.frames + ((int64_t)row * a.FR + fslot) * N;
    const float *__restrict__ w = tb.window;
    for (int i = threadIdx.x; i < N; i += nt) out[i] = fb[(i + hs) & (N - 1)] * w[i];
}

// --------------------------------------------------------------------------------------------
// synthesis, wave-per-frame variant.  The wave-private LDS region is reused four times:
// [output phases + rot/peak lists] -> [spectrum X] -> [butterfly-ordered input] -> [time-domain frame].
// --------------------------------------------------------------------------------------------
// kSink: 0 = the windowed frame goes to the HBM frame ring (a.frames); 1 = the un-windowed, un-shifted time-domain
// frame stays in the wave's LDS region (element e at lds[W::pad(e)] = samples 2e, 2e + 1) for the fused
// overlap-add that follows in the same kernel (pv_synth_chain_kernel)
// kFast: PV_ARITH_FAST (include/audiomod_pv.h) -- behind the phase propagation the output is continuous in everything
// computed here, so the arithmetic is free within the 1e-4 RMS contract: the region rotation is added without the
// wrap (sine and cosine do not care), sine / cosine come from the hardware's v_sin_f32 / v_cos_f32 (argument in turns),
// complex products use fma, and the first FFT pass multiplies by literal twiddles (pv_wavefft.h).  ~30 % fewer vector
// instructions per slice; measured against the oracle: see tests/test_gpu_parity.py (fast arithmetic) and bench.py.
template <int NC, int kPlainCore = -1, int kSink = 0, bool kFast = false>
__device__ __forceinline__ void synth_wave_role(const SynthArgs &a_in, const int row, const int tl, cf *lds,
                                                const int lane_in = -1) {
    // kPlainCore >= 0: the plain pitch shift / stretch in that core mode (no frequency compression, vocoder,
    // robotic, whisper or pass-through source): the mode switches fold away, the kernel is half the code
    SynthArgs a = a_in;
    if (kPlainCore >= 0) {
        a.do_freq_comp = 0, a.voc_band_len = -1, a.robotic = 0, a.passthru = 0, a.whisper = nullptr;
        a.coremode = kPlainCore;
    }
    // kPlainCore == 3: the formant / gender modes in the phase-locked core mode (frequency compression on, every
    // other switch off), for the fused kernel: with twelve waves per workgroup it has the registers (round 1's fold
    // spilled at 128)
    if (kPlainCore == 3) a.do_freq_comp = 1, a.coremode = 1;
    using W = WF<NC>;
    constexpr int N = 2 * NC, hs = NC, R = W::R;
    // (a caller that loops over slices passes a lane id that is opaque per iteration, so that the lane-dependent
    // addresses and constants below are not hoisted out of its loop and kept in registers across iterations)
    const int lane = lane_in >= 0 ? lane_in : (int)(threadIdx.x & 63);
    const DevTables &tb = a.tb;
    const int64_t t = a.t0 + tl;
    const int64_t plane = (int64_t)row * a.TR + ring_slot(a.s0, tl, a.TR);
    const float *__restrict__ mag = a.mag + plane * tb.HP;
    const float *__restrict__ A = a.phase + plane * tb.HP;
    const cf *__restrict__ tw = reinterpret_cast<const cf *>(tb.tw_inv);
    const cf *__restrict__ stw = reinterpret_cast<const cf *>(tb.st_inv);
    const cf2 *__restrict__ twl = reinterpret_cast<const cf2 *>(tb.twl_inv);
    const double Nd = (double)N;
    float *sph = reinterpret_cast<float *>(lds);                    // [hs + 1]
    float *srot = sph + hs + 4;                                     // [PKP]
    uint16_t *spk = reinterpret_cast<uint16_t *>(srot + a.PKP);     // [PKP]
    constexpr int JB = NC / 64; // bins per lane (plus the Nyquist bin on lane 0)

    // 1. every global value this frame needs, requested before anything is computed: the per-bin phases of
    //    whichever source the mode selects, the magnitudes, and (phase-locked steps) the peak list and its
    //    rotations, read speculatively up to the list's capacity so that they do not wait for the peak count.
    const int cslot = ring_slot(a.s0, tl, a.TR);
    constexpr int QP = (NC / 3 + 9 + 63) / 64; // >= PKP / 64 (pv_engine.cc: pkmax = hs / 3 + 2)
    const bool plain = !a.do_freq_comp && a.voc_band_len < 0; // magnitudes are used bin by bin, unmoved
    const float *__restrict__ psrc = A;
    int mode = kModeProp, n = 0;
    bool zero_phase = false;
    if (a.voc_band_len >= 0) {
        psrc = a.cphase + (int64_t)cslot * tb.HP;
    } else if (a.robotic) {
        zero_phase = true;
    } else if (a.passthru) {
    } else if (a.whisper) {
        psrc = a.whisper + ((int64_t)tl * a.C + row % a.C) * tb.HP;
    } else if (a.coremode == 2) {
    } else {
        mode = a.coremode == 1 ? a.modes[plane] : kModeProp;
        if (mode == kModeLock) n = a.npk[plane];
        else psrc = a.outphase + plane * tb.HP;
    }
    // A lane owns runs of four consecutive bins, k = 4 (lane + 64 q) + c: one 16-byte load per run and plane
    // (the texture path is issue-bound), and the spectrum goes to LDS as two 16-byte writes per run.
    constexpr int QB = NC / 256; // runs per lane
    constexpr int QH = (QB + 1) / 2; // magnitude runs fetched up front (the rest while those are being used)
    float4 base[QB], mreg[QB];
#pragma unroll
    for (int q = 0; q < QB; ++q) base[q] = *reinterpret_cast<const float4 *>(psrc + 4 * (lane + 64 * q));
    // the Nyquist bin keeps its analysis phase in every mode but the carrier / whisper / robotic ones (:695-699)
    float pnyq = (a.voc_band_len >= 0 || a.whisper) ? psrc[hs] : A[hs];
    float mnyq = 0.f;
    auto load_mags = [&]() { // issued once the peak list has left its registers (128-VGPR budget)
        if (plain) { // the first half now, the second half while the first is being used (see below)
#pragma unroll
            for (int q = 0; q < QH; ++q) mreg[q] = *reinterpret_cast<const float4 *>(mag + 4 * (lane + 64 * q));
            mnyq = mag[hs];
        } else if (a.do_freq_comp) { // freqCompSlice gathers across bins: the whole row, staged in LDS below
#pragma unroll
            for (int q = 0; q < QB; ++q) mreg[q] = *reinterpret_cast<const float4 *>(mag + 4 * (lane + 64 * q));
            mnyq = mag[hs];
        }
    };
    uint16_t pkr[QP];
    float rotr[QP];
    if (mode == kModeLock) {
#pragma unroll
        for (int q = 0; q < QP; ++q) {
            const int i = lane + 64 * q;
            const int ic = i < a.PKP ? i : 0;
            pkr[q] = a.peaks[plane * a.PKP + ic];
            rotr[q] = a.rot[plane * a.PKP + ic];
        }
    }

    // 2. output phase of every bin, in registers (and in sph for the modes that gather across bins)
    if (mode != kModeLock) load_mags();
    if (zero_phase) {
#pragma unroll
        for (int q = 0; q < QB; ++q) base[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        pnyq = 0.f;
    } else if (a.coremode == 2 && !a.passthru && !a.whisper && a.voc_band_len < 0) {
        const float pinc_f = (float)a.phase_inc[tl], hop_f = (float)a.hop;
#pragma unroll
        for (int q = 0; q < QB; ++q)
            base[q] = make_float4(base[q].x * pinc_f / hop_f, base[q].y * pinc_f / hop_f, base[q].z * pinc_f / hop_f,
                                  base[q].w * pinc_f / hop_f);
    } else if (mode == kModeLock) {
        // region(k) = number of region boundaries <= k.  Boundaries go into a bitmap (one 64-bit word per
        // 64 bins), so the lookup is a prefix count + one masked popcount per bin.
        unsigned int *bits32 = reinterpret_cast<unsigned int *>(spk + a.PKP); // [2 * JB]
        int *pre = reinterpret_cast<int *>(bits32 + 2 * JB);                  // [JB]
#pragma unroll
        for (int q = 0; q < QP; ++q) {
            const int i = lane + 64 * q;
            if (i < n) {
                spk[i] = pkr[q];
                srot[i] = rotr[q];
            }
        }
        load_mags();
        if (lane < 2 * JB) bits32[lane] = 0u;
        wave_sync();
        for (int i = lane; i + 1 < n; i += 64) {
            const int b = ((int)spk[i] + (int)spk[i + 1] + 1) >> 1; // round(x.5) away from zero (:676-682)
            atomicOr(&bits32[b >> 5], 1u << (b & 31));
        }
        wave_sync();
        const unsigned long long *bits = reinterpret_cast<const unsigned long long *>(bits32);
        if (lane < JB) {
            int acc = 0;
            for (int i = 0; i < lane; ++i) acc += __popcll(bits[i]);
            pre[lane] = acc;
        }
        wave_sync();
        const int b0 = 4 * (lane & 15); // bit of the run's first bin in its 64-bin word
#pragma unroll
        for (int q = 0; q < QB; ++q) {
            const int wd = (lane >> 4) + 4 * q; // == (4 (lane + 64 q)) >> 6
            const unsigned long long word = bits[wd];
            const int p0 = pre[wd];
            auto rotated = [&](float ph, int c) -> float {
                const int reg = p0 + __popcll(word & ((2ull << (b0 + c)) - 1ull));
                if (kFast) return ph + srot[reg]; // |.| <= 2 pi: the wrap only matters to a comparison, not to sin / cos
                return (float)princarg_small((double)(ph + srot[reg]));
            };
            base[q] = make_float4(rotated(base[q].x, 0), rotated(base[q].y, 1), rotated(base[q].z, 2),
                                  rotated(base[q].w, 3));
        }
    }
    float *smg = sph + hs + 4; // [hs + 1] magnitudes for the gather (over the rotation / peak lists, done with)
    if (!plain) {
        wave_sync();
#pragma unroll
        for (int q = 0; q < QB; ++q) *reinterpret_cast<float4 *>(sph + 4 * (lane + 64 * q)) = base[q];
        if (lane == 0) sph[hs] = pnyq;
        if (a.do_freq_comp) {
#pragma unroll
            for (int q = 0; q < QB; ++q) *reinterpret_cast<float4 *>(smg + 4 * (lane + 64 * q)) = mreg[q];
            if (lane == 0) smg[hs] = mnyq;
        }
        wave_sync();
    }

    // spectrum in registers: freqCompSlice gather (:869-916), gains, polar -> cartesian (FFT.cc:2711-2718)
    cf xs[QB][4];
    cf xnyq = cf{0.f, 0.f};
    auto to_cartesian = [&](float mg, float p) -> cf {
        mg *= a.inv_n;
        float sn, cs;
        if (kFast) { // phases unwrapped by freqCompSlice reach hundreds of radians: two-term reduction, then turns
            const float n = __builtin_rintf(p * 0.15915494309189535f);
            float r = __builtin_fmaf(n, -6.2831854820251465f, p);
            r = __builtin_fmaf(n, 1.7484555e-07f, r);
            const float rev = r * 0.15915494309189535f;
            sn = __builtin_amdgcn_sinf(rev), cs = __builtin_amdgcn_cosf(rev);
        } else {
            sincosf(p, &sn, &cs);
        }
        return cf{mg * cs, mg * sn};
    };
    auto spectrum_bin = [&](int k) -> cf {
        float mg, p;
        if (a.do_freq_comp) {
            if (a.freq_comp > 1.0f) {
                const int src = __float2int_rn((float)k * a.freq_comp);
                if (src > hs) {
                    mg = 0.f;
                    p = 0.f;
                } else {
                    mg = smg[src];
                    p = sph[src] + (float)((a.two_pi_hop * (double)(k - src)) / Nd);
                }
            } else if (k < hs) {
                const int src = __float2int_rn((float)k * a.freq_comp);
                mg = smg[src];
                p = sph[src] + (float)((a.two_pi_hop * (double)(k - src)) / Nd);
            } else {
                mg = smg[k];
                p = sph[k];
            }
            mg *= a.fixed_gain;
        } else {
            mg = vocoder_mag(mag, a.cmag + (int64_t)cslot * tb.HP, k, hs, a.voc_band_len);
            p = sph[k];
        }
        return to_cartesian(mg, p);
    };
    if (plain) {
        // The phases of the plain modes are wrapped (or a small multiple of a wrapped phase, core mode 2): the short
        // sine / cosine of pv_sincos.h serves them; one wave-uniform test of the run's sixteen phases keeps the
        // device library's for anything beyond its argument bound (and for NaN, which fails the comparison).
        float pmax = __builtin_fabsf(pnyq);
#pragma unroll
        for (int q = 0; q < QB; ++q)
            pmax = __builtin_fmaxf(__builtin_fmaxf(pmax, pv_max3_abs(base[q].x, base[q].y, base[q].z)), __builtin_fabsf(base[q].w));
        auto to_cartesian_small = [&](float mg, float p) -> cf {
            mg *= a.inv_n;
            float sn, cs;
            if (kFast) { // |p| is a few turns at most: v_sin_f32 / v_cos_f32 take turns, valid to +-256
                const float rev = p * 0.15915494309189535f;
                sn = __builtin_amdgcn_sinf(rev), cs = __builtin_amdgcn_cosf(rev);
            } else {
                pv_sincos_small(p, sn, cs);
            }
            return cf{mg * cs, mg * sn};
        };
        if (kFast || __builtin_amdgcn_ballot_w64(!(pmax <= PV_SINCOS_MAX_ARG)) == 0) {
#pragma unroll
            for (int q = 0; q < QB; ++q) {
                if (q + QH < QB) mreg[q + QH] = *reinterpret_cast<const float4 *>(mag + 4 * (lane + 64 * (q + QH)));
                xs[q][0] = to_cartesian_small(mreg[q].x, base[q].x);
                xs[q][1] = to_cartesian_small(mreg[q].y, base[q].y);
                xs[q][2] = to_cartesian_small(mreg[q].z, base[q].z);
                xs[q][3] = to_cartesian_small(mreg[q].w, base[q].w);
            }
            if (lane == 0) xnyq = to_cartesian_small(mnyq, pnyq);
        } else {
#pragma unroll
            for (int q = 0; q < QB; ++q) {
                if (q + QH < QB) mreg[q + QH] = *reinterpret_cast<const float4 *>(mag + 4 * (lane + 64 * (q + QH)));
                xs[q][0] = to_cartesian(mreg[q].x, base[q].x);
                xs[q][1] = to_cartesian(mreg[q].y, base[q].y);
                xs[q][2] = to_cartesian(mreg[q].z, base[q].z);
                xs[q][3] = to_cartesian(mreg[q].w, base[q].w);
            }
            if (lane == 0) xnyq = to_cartesian(mnyq, pnyq);
        }
    } else {
#pragma unroll
        for (int q = 0; q < QB; ++q)
#pragma unroll
            for (int c = 0; c < 4; ++c) xs[q][c] = spectrum_bin(4 * (lane + 64 * q) + c);
        if (lane == 0) xnyq = spectrum_bin(hs);
    }
    wave_sync();
#pragma unroll
    for (int q = 0; q < QB; ++q) {
        float4 *dst = reinterpret_cast<float4 *>(lds + 4 * (lane + 64 * q));
        dst[0] = make_float4(xs[q][0].x, xs[q][0].y, xs[q][1].x, xs[q][1].y);
        dst[1] = make_float4(xs[q][2].x, xs[q][2].y, xs[q][3].x, xs[q][3].y);
    }
    if (lane == 0) lds[hs] = xnyq;
    wave_sync();

    // 3. kiss_fftri pre-pass (kiss_fftr.c:134-157): pairs (k, NC-k) into registers, then scattered into
    //    butterfly order.  k = lane + 64 j; NC - k = 64 * (JB - j - (lane != 0)) + ((64 - lane) & 63).
    constexpr int J = NC / 128;
    constexpr bool kRoomy = NC <= 1024; // registers to spare for the earlier of two possible issue points
    cf sw[J];
    if (kRoomy) {
#pragma unroll
        for (int j = 0; j < J; ++j) sw[j] = stw[lane + 64 * j];
    }
    const cf swmid = stw[NC / 2];
    WfTw<W> T0, T1, T2;
    WfTwRaw<W, 1> raw1;
    if (kRoomy) {
        if (!(kFast && wf_pass_all_const<W, 0>())) wf_load_pass_tw<W, 0>(T0, lane, tw); // (fast: literal twiddles)
        wf_fetch_pass_tw<W, 1>(raw1, lane, twl);
    }
    cf pa[J], pb[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int k = lane + 64 * j;
        pa[j] = lds[k];
        pb[j] = lds[NC - k];
    }
    const cf pmid = lds[NC / 2];
    wave_sync();
    const int e_lane = wf_e_of_src<W>(lane);             // low six source bits
    const int e_lane2 = wf_e_of_src<W>((64 - lane) & 63);
#pragma unroll
    for (int j = 0; j < J; ++j) {
        if (j == 0 && lane == 0) {
            lds[W::pad(wf_e_of_src<W>(0))] = cf{pa[0].x + pb[0].x, pa[0].x - pb[0].x};
        } else {
            const cf fk = pa[j];
            const cf fnkc = cf{pb[j].x, -pb[j].y};
            const cf fek = wf_add(fk, fnkc);
            const cf tq = wf_sub(fk, fnkc);
            const cf fok = kFast ? wf_cmul_fma(tq, kRoomy ? sw[j] : stw[lane + 64 * j])
                                 : wf_cmul(tq, kRoomy ? sw[j] : stw[lane + 64 * j]);
            const cf u = wf_add(fek, fok);
            cf vv = wf_sub(fek, fok);
            vv.y = vv.y * -1.f;
            const int e1 = e_lane | wf_e_of_src<W>(64 * j);
            const int hi2 = lane != 0 ? wf_e_of_src<W>(64 * (JB - j - 1)) : wf_e_of_src<W>((64 * (JB - j)) & (NC - 1));
            const int e2 = e_lane2 | hi2;
            lds[W::pad(e1)] = u;
            lds[W::pad(e2)] = vv;
        }
    }
    if (lane == 0) { // k == NC/2: only the second assignment survives
        const cf fk = pmid;
        const cf fnkc = cf{pmid.x, -pmid.y};
        const cf fek = wf_add(fk, fnkc);
        const cf tq = wf_sub(fk, fnkc);
        const cf fok = wf_cmul(tq, swmid);
        cf vv = wf_sub(fek, fok);
        vv.y = vv.y * -1.f;
        lds[W::pad(wf_e_of_src<W>(NC / 2))] = vv;
    }
    wave_sync();

    // 4. inverse complex FFT.  With registers to spare (N = 2048: 125 VGPRs, four waves per SIMD) the twiddles
    //    are fetched a pass ahead and the synthesis window before the frame's first store (see the analysis
    //    kernel); at N = 4096 the 32 values per lane leave no room for that and every load sits at its use.
    cf v[R];
    {
        const int lp = wf_lane_part<W>(0, lane);
#pragma unroll
        for (int r = 0; r < R; ++r) v[r] = lds[W::pad(lp | wf_reg_part<W>(0, r))];
    }
    const int fslot = (int)(t & (int64_t)(a.FR - 1));
    float *__restrict__ out = a.frames + ((int64_t)row * a.FR + fslot) * N;
    const float *__restrict__ w = tb.window;
    if constexpr (kRoomy) {
        const int lp0 = wf_lane_part<W>(0, lane), lp1 = wf_lane_part<W>(1, lane), lp2 = wf_lane_part<W>(2, lane);
        wave_sync();
        if (kFast) wf_apply_pass_stages_fast<W, 0, true>(v, T0);
        else wf_apply_pass_stages<W, 0, true>(v, T0);
        wf_store<W, 0>(lds, v, lp0);
        wave_sync();
        wf_load<W, 1>(lds, v, lp1);
        wf_unpack_pass_tw<W, 1>(T1, raw1);
        if (kFast) wf_apply_pass_stages_fast<W, 1, true>(v, T1);
        else wf_apply_pass_stages<W, 1, true>(v, T1);
        WfTwRaw<W, 2> raw2;
        wf_fetch_pass_tw<W, 2>(raw2, lane, twl);
        wf_store<W, 1>(lds, v, lp1);
        wave_sync();
        wf_load<W, 2>(lds, v, lp2);
        wf_unpack_pass_tw<W, 2>(T2, raw2);
        if (kFast) wf_apply_pass_stages_fast<W, 2, true>(v, T2);
        else wf_apply_pass_stages<W, 2, true>(v, T2);
        constexpr int PL = W::NPASS - 1; // the last pass
        const int lpl = wf_lane_part<W>(PL, lane);
        if constexpr (W::NPASS == 4) { // (512 points: the last radix-4 stage is a pass of its own)
            WfTwRaw<W, 3> raw3;
            wf_fetch_pass_tw<W, 3>(raw3, lane, twl);
            wf_store<W, 2>(lds, v, lp2);
            wave_sync();
            wf_load<W, 3>(lds, v, lpl);
            wf_unpack_pass_tw<W, 3>(T1, raw3);
            if (kFast) wf_apply_pass_stages_fast<W, 3, true>(v, T1);
            else wf_apply_pass_stages<W, 3, true>(v, T1);
        }
        if constexpr (kSink == 1) {
            wf_store<W, PL>(lds, v, lpl);
            wave_sync();
            return;
        }
        float4 ww[NC / 128];
#pragma unroll
        for (int j = 0; j < NC / 128; ++j) ww[j] = *reinterpret_cast<const float4 *>(w + 4 * (lane + 64 * j));
        wf_store<W, PL>(lds, v, lpl);
        wave_sync();
        // 5. ifftshift + synthesis window (phasevocoderimpl.h:183-198): four consecutive samples per lane and
        //    store (the stores are issue-bound: half as many 16-byte ones beat twice as many 8-byte ones)
#pragma unroll
        for (int j = 0; j < NC / 128; ++j) {
            const int i = 4 * (lane + 64 * j);        // output sample index
            const int e = ((i + hs) & (N - 1)) >> 1;  // even: elements e, e+1 hold samples i+hs .. i+hs+3
            const cf z0 = lds[W::pad(e)], z1 = lds[W::pad(e) + 1]; // same group of 16, so adjacent after padding
            *reinterpret_cast<float4 *>(out + i) =
                make_float4(z0.x * ww[j].x, z0.y * ww[j].y, z1.x * ww[j].z, z1.y * ww[j].w);
        }
    } else {
        // no room to fetch a pass ahead, but the lane-major tables still turn each pass's twiddle gathers into a
        // few contiguous 16-byte loads
        wave_sync();
        if (kFast && wf_pass_all_const<W, 0>()) { // every twiddle of the pass is a literal: nothing to fetch
            wf_apply_pass_stages_fast<W, 0, true>(v, T0);
            wf_store<W, 0>(lds, v, wf_lane_part<W>(0, lane));
        } else {
            wf_fft_pass<W, 0, true>(v, lane, lds, tw);
        }
        wave_sync();
        {
            WfTwRaw<W, 1> r1;
            wf_fetch_pass_tw<W, 1>(r1, lane, twl);
            wf_unpack_pass_tw<W, 1>(T1, r1);
            if (kFast) {
                wf_load<W, 1>(lds, v, wf_lane_part<W>(1, lane));
                wf_apply_pass_stages_fast<W, 1, true>(v, T1);
                wf_store<W, 1>(lds, v, wf_lane_part<W>(1, lane));
            } else {
                wf_fft_pass_tw<W, 1, true>(v, lane, lds, T1);
            }
        }
        wave_sync();
        {
            WfTwRaw<W, 2> r2;
            wf_fetch_pass_tw<W, 2>(r2, lane, twl);
            wf_unpack_pass_tw<W, 2>(T2, r2);
            if (kFast) {
                wf_load<W, 2>(lds, v, wf_lane_part<W>(2, lane));
                wf_apply_pass_stages_fast<W, 2, true>(v, T2);
                wf_store<W, 2>(lds, v, wf_lane_part<W>(2, lane));
            } else {
                wf_fft_pass_tw<W, 2, true>(v, lane, lds, T2);
            }
        }
        if constexpr (kSink == 1) {
            wave_sync();
            return;
        }
        // (v is dead now: the whole window fits in its registers, fetched before the frame's first store, and the
        // frame leaves 16 bytes per lane like the other variant's)
        float4 ww[NC / 128];
#pragma unroll
        for (int j = 0; j < NC / 128; ++j) ww[j] = *reinterpret_cast<const float4 *>(w + 4 * (lane + 64 * j));
        wave_sync();
#pragma unroll
        for (int j = 0; j < NC / 128; ++j) {
            const int i = 4 * (lane + 64 * j);
            const int e = ((i + hs) & (N - 1)) >> 1;
            const cf z0 = lds[W::pad(e)], z1 = lds[W::pad(e) + 1];
            *reinterpret_cast<float4 *>(out + i) =
                make_float4(z0.x * ww[j].x, z0.y * ww[j].y, z1.x * ww[j].z, z1.y * ww[j].w);
        }
    }
}

// (N = 2048 is asked to fit four waves per SIMD, 128 VGPRs; the compiler gets there without spilling)
template <int NC, int WPB, int kPlainCore = -1>
__global__ __launch_bounds__(64 * WPB) __attribute__((amdgpu_waves_per_eu(NC == 1024 ? 4 : 1))) void
pv_synth_wave_kernel(const SynthArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    cf *lds = reinterpret_cast<cf *>(smem_raw) + (threadIdx.x >> 6) * WF<NC>::LDS_CF;
    int row, tl;
    if (!block_to_row_slice_w<WPB>(a.Tn, a.rows, row, tl)) return; // wave-uniform
    synth_wave_role<NC, kPlainCore>(a, row, tl, lds);
}

// AUDIOMOD_PV_SYNTH_GENERIC=1: every mode through the all-modes kernel (tests compare it with the specialisation)
static bool synth_generic_only() {
    static const bool on = [] {
        const char *e = getenv("AUDIOMOD_PV_SYNTH_GENERIC");
        return e && atoi(e) != 0;
    }();
    return on;
}

void launch_synth(const SynthArgs &a, hipStream_t st) {
    if (a.tb.nc == 512 || a.tb.nc == 256) { // fft 1024 / 512 (round 3): the phase-locked plain specialisation, else the all-modes kernel
        constexpr int WPB = 1;
        const int grid = 8 * ((a.rows + 7) / 8) * ((a.Tn + WPB - 1) / WPB);
        const bool plain = !a.do_freq_comp && a.voc_band_len < 0 && !a.robotic && !a.passthru && !a.whisper &&
                           !synth_generic_only();
        if (a.tb.nc == 512) {
            const size_t lds = WPB * WF<512>::LDS_CF * sizeof(cf);
            if (plain && a.coremode == 1) hipLaunchKernelGGL((pv_synth_wave_kernel<512, WPB, 1>), dim3(grid), dim3(64 * WPB), lds, st, a);
            else hipLaunchKernelGGL((pv_synth_wave_kernel<512, WPB>), dim3(grid), dim3(64 * WPB), lds, st, a);
        } else {
            const size_t lds = WPB * WF<256>::LDS_CF * sizeof(cf);
            if (plain && a.coremode == 1) hipLaunchKernelGGL((pv_synth_wave_kernel<256, WPB, 1>), dim3(grid), dim3(64 * WPB), lds, st, a);
            else hipLaunchKernelGGL((pv_synth_wave_kernel<256, WPB>), dim3(grid), dim3(64 * WPB), lds, st, a);
        }
        return;
    }
    if (a.tb.nc == 1024 || a.tb.nc == 2048) {
        if (a.tb.nc == 1024) {
            constexpr int WPB = 1;
            const int grid = 8 * ((a.rows + 7) / 8) * ((a.Tn + WPB - 1) / WPB);
            const bool plain = !a.do_freq_comp && a.voc_band_len < 0 && !a.robotic && !a.passthru && !a.whisper &&
                               !synth_generic_only();
            if (plain && a.coremode >= 0 && a.coremode <= 2) {
                const size_t lds = WPB * WF<1024>::LDS_CF * sizeof(cf);
                if (a.coremode == 1) hipLaunchKernelGGL((pv_synth_wave_kernel<1024, WPB, 1>), dim3(grid), dim3(64 * WPB), lds, st, a);
                else if (a.coremode == 0) hipLaunchKernelGGL((pv_synth_wave_kernel<1024, WPB, 0>), dim3(grid), dim3(64 * WPB), lds, st, a);
                else hipLaunchKernelGGL((pv_synth_wave_kernel<1024, WPB, 2>), dim3(grid), dim3(64 * WPB), lds, st, a);
                return;
            }
            launch_big_lds<pv_synth_wave_kernel<1024, WPB>>(dim3(grid), dim3(64 * WPB),
                               WPB * WF<1024>::LDS_CF * sizeof(cf), st, a);
        } else {
            constexpr int WPB = 1;
            const int grid = 8 * ((a.rows + 7) / 8) * ((a.Tn + WPB - 1) / WPB);
            const bool plain = !a.do_freq_comp && a.voc_band_len < 0 && !a.robotic && !a.passthru && !a.whisper &&
                               !synth_generic_only();
            if (plain && a.coremode >= 0 && a.coremode <= 2) {
                const size_t lds = WPB * WF<2048>::LDS_CF * sizeof(cf);
                if (a.coremode == 1) hipLaunchKernelGGL((pv_synth_wave_kernel<2048, WPB, 1>), dim3(grid), dim3(64 * WPB), lds, st, a);
                else if (a.coremode == 0) hipLaunchKernelGGL((pv_synth_wave_kernel<2048, WPB, 0>), dim3(grid), dim3(64 * WPB), lds, st, a);
                else hipLaunchKernelGGL((pv_synth_wave_kernel<2048, WPB, 2>), dim3(grid), dim3(64 * WPB), lds, st, a);
                return;
            }
            launch_big_lds<pv_synth_wave_kernel<2048, WPB>>(dim3(grid), dim3(64 * WPB),
                               WPB * WF<2048>::LDS_CF * sizeof(cf), st, a);
        }
        return;
    }
    const int grid = 8 * ((a.rows + 7) / 8) * a.Tn;
    const size_t lds = (size_t)(2 * a.tb.nc + 1) * sizeof(float2) + sizeof(float) * (a.tb.hs + 4 + a.PKP) +
                       sizeof(uint16_t) * a.PKP;
    launch_big_lds<pv_synth_kernel>(dim3(grid), dim3(generic_fft_threads(a.tb.nc)), lds, st, a);
}

// --------------------------------------------------------------------------------------------
// Cepstral formant shift of a slice's magnitudes (extension mode; the reference's formantShiftSlice,
// phasevocoderprocess.cc:925-999, with D_KISSFFT::inverseCepstral FFT.cc:2723-2733 and ::forward :2606-2610 --
// unreachable upstream, restated in oracle/pv_oracle.c formant_shift and pinned there on the real function):
//   cep = kiss_fftri(log(mag + 1e-6));  keep the first 60 quefrencies (ends halved), times 1/N;
//   envelope = exp(Re kiss_fftr(cep));  mag = mag / envelope * envelope[lrint(k * env_comp)]
// One wave per (row, slice), both transforms through the wave-FFT core in the wave's LDS region.
// --------------------------------------------------------------------------------------------
template <int NC>
__device__ __forceinline__ void cepstral_wave_role(const CepstralArgs &a, const int row, const int tl, cf *lds) {
    using W = WF<NC>;
    constexpr int hs = NC, R = W::R, J = NC / 128, QB = NC / 256, kCut = 60;
    const int lane = threadIdx.x & 63;
    const DevTables &tb = a.tb;
    const int64_t plane = (int64_t)row * a.TR + ring_slot(a.s0, tl, a.TR);
    float *__restrict__ mag = a.mag + plane * tb.HP;
    const cf *__restrict__ twi = reinterpret_cast<const cf *>(tb.tw_inv);
    const cf *__restrict__ twf = reinterpret_cast<const cf *>(tb.tw_fwd);
    const cf *__restrict__ sti = reinterpret_cast<const cf *>(tb.st_inv);
    const cf *__restrict__ stf = reinterpret_cast<const cf *>(tb.st_fwd);

    // magnitudes: runs of four consecutive bins per lane (kept in registers for the end), and the Nyquist bin
    float4 m4[QB];
#pragma unroll
    for (int q = 0; q < QB; ++q) m4[q] = *reinterpret_cast<const float4 *>(mag + 4 * (lane + 64 * q));
    const float mny = mag[hs];
    // X[k] = (logf(mag[k] + 1e-6), 0) in natural order
#pragma unroll
    for (int q = 0; q < QB; ++q) {
        float4 *dst = reinterpret_cast<float4 *>(lds + 4 * (lane + 64 * q));
        dst[0] = make_float4(logf(m4[q].x + 0.000001f), 0.f, logf(m4[q].y + 0.000001f), 0.f);
        dst[1] = make_float4(logf(m4[q].z + 0.000001f), 0.f, logf(m4[q].w + 0.000001f), 0.f);
    }
    const cf xnyq = cf{logf(mny + 0.000001f), 0.f};
    wave_sync();

    // kiss_fftri pre-pass (kiss_fftr.c:134-157), as in the synthesis kernel
    cf v[R];
    {
        cf pa[J], pb[J];
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int k = lane + 64 * j;
            pa[j] = lds[k];
            pb[j] = lds[(NC - k) & (NC - 1)];
        }
        if (lane == 0) pb[0] = xnyq;
        const cf pmid = lds[NC / 2];
        wave_sync();
        const int e_lane = wf_e_of_src<W>(lane);
        const int e_lane2 = wf_e_of_src<W>((64 - lane) & 63);
        constexpr int JB = NC / 64;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            if (j == 0 && lane == 0) {
                lds[W::pad(wf_e_of_src<W>(0))] = cf{pa[0].x + pb[0].x, pa[0].x - pb[0].x};
            } else {
                const cf fk = pa[j];
                const cf fnkc = cf{pb[j].x, -pb[j].y};
                const cf fek = wf_add(fk, fnkc);
                const cf tq = wf_sub(fk, fnkc);
                const cf fok = wf_cmul(tq, sti[lane + 64 * j]);
                const cf u = wf_add(fek, fok);
                cf vv = wf_sub(fek, fok);
                vv.y = vv.y * -1.f;
                const int e1 = e_lane | wf_e_of_src<W>(64 * j);
                const int hi2 = lane != 0 ? wf_e_of_src<W>(64 * (JB - j - 1)) : wf_e_of_src<W>((64 * (JB - j)) & (NC - 1));
                const int e2 = e_lane2 | hi2;
                lds[W::pad(e1)] = u;
                lds[W::pad(e2)] = vv;
            }
        }
        if (lane == 0) {
            const cf fk = pmid;
            const cf fnkc = cf{pmid.x, -pmid.y};
            const cf fek = wf_add(fk, fnkc);
            const cf tq = wf_sub(fk, fnkc);
            const cf fok = wf_cmul(tq, sti[NC / 2]);
            cf vv = wf_sub(fek, fok);
            vv.y = vv.y * -1.f;
            lds[W::pad(wf_e_of_src<W>(NC / 2))] = vv;
        }
        wave_sync();
        const int lp = wf_lane_part<W>(0, lane);
#pragma unroll
        for (int r = 0; r < R; ++r) v[r] = lds[W::pad(lp | wf_reg_part<W>(0, r))];
    }
    wave_sync();
    wf_fft_pass<W, 0, true>(v, lane, lds, twi);
    wave_sync();
    wf_fft_pass<W, 1, true>(v, lane, lds, twi);
    wave_sync();
    wf_fft_pass<W, 2, true>(v, lane, lds, twi);
    wave_sync();
    if constexpr (W::NPASS == 4) { // (256 / 512 points: the last radix-4 stage is a pass of its own)
        wf_fft_pass<W, 3, true>(v, lane, lds, twi);
        wave_sync();
    }

    // lifter: element e of the transform holds cep[2e], cep[2e+1]; only the first 60 survive
    cf z = cf{0.f, 0.f};
    if (lane < kCut / 2) {
        z = lds[W::pad(lane)];
        if (lane == 0) z.x = z.x / 2;
        if (lane == kCut / 2 - 1) z.y = z.y / 2;
        z.x = z.x * a.inv_n;
        z.y = z.y * a.inv_n;
    }
    wave_sync();
    cf *zl = lds + W::LDS_CF - 32; // scratch at the end of the region (consumed before the next pass writes there)
    if (lane < 32) zl[lane] = z;
    wave_sync();
    // forward transform of the zero-extended sequence: pass-0 layout straight from the 32 survivors
    {
        const int lp = wf_lane_part<W>(0, lane);
        const int lsrc = wf_src_of<W>(lp);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int src = lsrc | wf_src_of_const<W>(wf_reg_part<W>(0, r));
            const cf t = zl[src & 31];
            v[r] = src < 32 ? t : cf{0.f, 0.f};
        }
    }
    wave_sync();
    wf_fft_pass<W, 0, false>(v, lane, lds, twf);
    wave_sync();
    wf_fft_pass<W, 1, false>(v, lane, lds, twf);
    wave_sync();
    wf_fft_pass<W, 2, false>(v, lane, lds, twf);
    wave_sync();
    if constexpr (W::NPASS == 4) {
        wf_fft_pass<W, 3, false>(v, lane, lds, twf);
        wave_sync();
    }

    // real parts of the real-FFT split (kiss_fftr.c:91-120), exponentiated: the spectral envelope
    float elo[J], ehi[J], emid = 0.f;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int k = lane + 64 * j;
        if (j == 0 && lane == 0) {
            const cf tdc = lds[W::pad(0)];
            elo[0] = expf(tdc.x + tdc.y);
            ehi[0] = expf(tdc.x - tdc.y);
        } else {
            const cf fpk = lds[W::pad(k)];
            const cf q = lds[W::pad(NC - k)];
            const cf fpnk = cf{q.x, -q.y};
            const cf f1k = wf_add(fpk, fpnk);
            const cf f2k = wf_sub(fpk, fpnk);
            const cf tq = wf_cmul(f2k, stf[k]);
            elo[j] = expf((f1k.x + tq.x) * 0.5f);
            ehi[j] = expf((f1k.x - tq.x) * 0.5f);
        }
    }
    if (lane == 0) {
        const cf fpk = lds[W::pad(NC / 2)];
        const cf fpnk = cf{fpk.x, -fpk.y};
        const cf f1k = wf_add(fpk, fpnk);
        const cf f2k = wf_sub(fpk, fpnk);
        const cf tq = wf_cmul(f2k, stf[NC / 2]);
        emid = expf((f1k.x - tq.x) * 0.5f);
    }
    wave_sync();
    float *senv = reinterpret_cast<float *>(lds); // [hs + 1]
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int k = lane + 64 * j;
        if (j == 0 && lane == 0) {
            senv[0] = elo[0];
            senv[NC] = ehi[0];
        } else {
            senv[k] = elo[j];
            senv[NC - k] = ehi[j];
        }
    }
    if (lane == 0) senv[NC / 2] = emid;
    wave_sync();

    // whiten by the envelope, re-colour by the envelope read at lrint(k * env_comp)
    auto shifted = [&](int k) -> float {
        if (a.env_comp > 1.0f) {
            const int src = __float2int_rn((float)k * a.env_comp);
            return src > hs ? 0.f : senv[src];
        }
        if (k == hs) return senv[hs]; // the downward loop of the reference never touches the Nyquist bin
        return senv[__float2int_rn((float)k * a.env_comp)];
    };
#pragma unroll
    for (int q = 0; q < QB; ++q) {
        const int k0 = 4 * (lane + 64 * q);
        const float4 e4 = *reinterpret_cast<const float4 *>(senv + k0);
        float4 o;
        o.x = (m4[q].x / e4.x) * shifted(k0);
        o.y = (m4[q].y / e4.y) * shifted(k0 + 1);
        o.z = (m4[q].z / e4.z) * shifted(k0 + 2);
        o.w = (m4[q].w / e4.w) * shifted(k0 + 3);
        *reinterpret_cast<float4 *>(mag + k0) = o;
    }
    if (lane == 0) mag[hs] = (mny / senv[hs]) * shifted(hs);
}

template <int NC> __global__ __launch_bounds__(64) void pv_cepstral_wave_kernel(const CepstralArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    int row, tl;
    if (!block_to_row_slice_w<1>(a.Tn, a.rows, row, tl)) return; // wave-uniform
    cepstral_wave_role<NC>(a, row, tl, reinterpret_cast<cf *>(smem_raw));
}

// Any FFT size (round 2): one workgroup per (row, slice), both transforms through the generic LDS butterfly stages --
// the same steps as the wave version above, the same arithmetic as the reference's formantShiftSlice
// (phasevocoderprocess.cc:925-999), which is size-agnostic.
__global__ __launch_bounds__(kFftThreads) void pv_cepstral_kernel(const CepstralArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    const DevTables &tb = a.tb;
    const int hs = tb.hs, nc = tb.nc, nt = blockDim.x;
    constexpr int kCut = 60;
    float2 *buf = reinterpret_cast<float2 *>(smem_raw); // [nc]      butterfly array
    float2 *X = buf + nc;                               // [nc + 1]  log-magnitude spectrum
    float *senv = reinterpret_cast<float *>(X + nc + 1); // [hs + 1] envelope
    float *scep = senv + hs + 4;                        // [64]      the surviving quefrencies
    int row, tl;
    if (!block_to_row_slice(a.Tn, a.rows, row, tl)) return;
    const int64_t plane = (int64_t)row * a.TR + ring_slot(a.s0, tl, a.TR);
    float *__restrict__ mag = a.mag + plane * tb.HP;
    for (int k = threadIdx.x; k <= hs; k += nt) X[k] = make_float2(logf(mag[k] + 0.000001f), 0.f);
    __syncthreads();
    // kiss_fftri pre-pass (kiss_fftr.c:134-157) scattered into butterfly order, inverse stages: buf = cep pairs
    for (int k = threadIdx.x; k <= nc / 2; k += nt) {
        if (k == 0) {
            buf[tb.iperm[0]] = make_float2(X[0].x + X[nc].x, X[0].x - X[nc].x);
        } else {
            const float2 fk = X[k];
            const float2 q = X[nc - k];
            const float2 fnkc = make_float2(q.x, -q.y);
            const float2 fek = cadd(fk, fnkc);
            const float2 tq = csub(fk, fnkc);
            const float2 fok = cmul(tq, tb.st_inv[k]);
            const float2 u = cadd(fek, fok);
            float2 v = csub(fek, fok);
            v.y = v.y * -1.f;
            if (k != nc - k) buf[tb.iperm[k]] = u;
            buf[tb.iperm[nc - k]] = v;
        }
    }
    __syncthreads();
    fft_stages<true>(buf, tb, tb.tw_inv);
    // lifter: the first 60 quefrencies survive, the two ends halved, all times 1 / N (:952-960)
    if (threadIdx.x < 64) {
        const float *cep = reinterpret_cast<const float *>(buf);
        float c = threadIdx.x < kCut ? cep[threadIdx.x] : 0.f;
        if (threadIdx.x == 0 || threadIdx.x == kCut - 1) c = c / 2;
        scep[threadIdx.x] = threadIdx.x < kCut ? c * a.inv_n : 0.f;
    }
    __syncthreads();
    // forward real transform of the zero-extended sequence (kiss_fftr.c:67-121): pairs in butterfly order
    for (int j = threadIdx.x; j < nc; j += nt) {
        const int src = tb.perm[j];
        buf[j] = src < 32 ? make_float2(scep[2 * src], scep[2 * src + 1]) : make_float2(0.f, 0.f);
    }
    __syncthreads();
    fft_stages<false>(buf, tb, tb.tw_fwd);
    for (int k = threadIdx.x; k <= nc / 2; k += nt) {
        if (k == 0) {
            const float2 tdc = buf[0];
            senv[0] = expf(tdc.x + tdc.y);
            senv[nc] = expf(tdc.x - tdc.y);
        } else {
            const float2 fpk = buf[k];
            const float2 q = buf[nc - k];
            const float2 fpnk = make_float2(q.x, -q.y);
            const float2 f1k = cadd(fpk, fpnk);
            const float2 f2k = csub(fpk, fpnk);
            const float2 tq = cmul(f2k, tb.st_fwd[k]);
            if (k != nc - k) senv[k] = expf((f1k.x + tq.x) * 0.5f);
            senv[nc - k] = expf((f1k.x - tq.x) * 0.5f);
        }
    }
    __syncthreads();
    // whiten by the envelope, re-colour by the envelope read at lrint(k * env_comp) (:962-998)
    for (int k = threadIdx.x; k <= hs; k += nt) {
        float sh;
        if (a.env_comp > 1.0f) {
            const int src = __float2int_rn((float)k * a.env_comp);
            sh = src > hs ? 0.f : senv[src];
        } else if (k == hs) {
            sh = senv[hs]; // the downward loop of the reference never touches the Nyquist bin
        } else {
            sh = senv[__float2int_rn((float)k * a.env_comp)];
        }
        mag[k] = (mag[k] / senv[k]) * sh;
    }
}

// (the census of the launchers' choices, below: which cepstral kernel a launch is)
static void census_cepstral(int set, int kernel, int nc);

void launch_cepstral(const CepstralArgs &a, hipStream_t st) {
    const int grid = 8 * ((a.rows + 7) / 8) * a.Tn;
    census_cepstral(0, a.tb.nc != 1024 && a.tb.nc != 2048 ? kCepKernelGeneric : kCepKernelWave, a.tb.nc);
    if (a.tb.nc != 1024 && a.tb.nc != 2048) {
        const size_t lds = (size_t)(2 * a.tb.nc + 1) * sizeof(float2) + sizeof(float) * (a.tb.hs + 4 + 64);
        launch_big_lds<pv_cepstral_kernel>(dim3(grid), dim3(generic_fft_threads(a.tb.nc)), lds, st, a);
        return;
    }
    if (a.tb.nc == 1024) {
        hipLaunchKernelGGL((pv_cepstral_wave_kernel<1024>), dim3(grid), dim3(64), WF<1024>::LDS_CF * sizeof(cf), st, a);
    } else {
        hipLaunchKernelGGL((pv_cepstral_wave_kernel<2048>), dim3(grid), dim3(64), WF<2048>::LDS_CF * sizeof(cf), st, a);
    }
}

// --------------------------------------------------------------------------------------------
// overlap-add + normalise + resample
// --------------------------------------------------------------------------------------------
typedef float v2f __attribute__((ext_vector_type(2)));

// NR rows (stream-channels) per workgroup.  All rows share one schedule, so a tile's descriptor, its frame
// offsets, its output table and -- in the resampler -- the coefficient row of an output are the same for every row:
// with NR = 2 a workgroup fetches them once for two rows, each resampler thread reads a coefficient once for two
// outputs (the loop is bound by LDS reads), and the dependent chain descriptor -> offsets -> frame gather ->
// resample, which at full occupancy is what the kernel waits on, is paid once for twice the work.
// kRes: -1 = resampling mode read from the arguments; 0 = none, 1 = direct sinc table, 2 = cubic-interpolated table
// (the argument's flags become compile-time constants)
template <int NR, int kRes = -1>
__device__ __forceinline__ void ola_role(const OlaArgs &a_in, const int tile_i, const int row0, char *smem_raw) {
    OlaArgs a = a_in;
    if (kRes >= 0) a.resample = kRes != 0, a.interp = kRes == 2;
    // interpolated mode: coefficient table expanded per sub-sample offset, tab4[off][j] = the four taps
    // sinc[4 + (j+1)*ov - off + {-2,-1,0,1}] of resampler_basic_interpolate_single (resample.c:494-535) as one
    // aligned float4; rows are padded to NF+1 slots so the (at most ov) distinct rows a wave reads in one
    // ds_read_b128 land on different banks.  direct mode: the sinc table as it is.
    float4 *tab4 = reinterpret_cast<float4 *>(smem_raw);
    float *stab = reinterpret_cast<float *>(smem_raw);
    float *ola = reinterpret_cast<float *>(smem_raw + a.tab_bytes);   // [NR][lds_floats]
    int *sP = reinterpret_cast<int *>(ola + NR * a.lds_floats);       // [kMaxTileFrames] P_t - n_lo
    const int nt = blockDim.x, tid = threadIdx.x;
    const OlaTile tile = a.tiles[tile_i];
    const int N = a.N, NF = a.filt_len;

    // position of this thread's output in the tile, its sub-sample offset and interpolation fraction: planned
    // on the host (pv_engine.cc build_tiles), one 8-byte entry per output, fetched ahead of the gather
    const float *__restrict__ wacc = a.wacc + (int64_t)tile_i * a.wacc_pitch;
    uint2 oe = make_uint2(0u, 0u);
    if (a.resample && tid < tile.kcnt) oe = reinterpret_cast<const uint2 *>(wacc + a.otab_off)[tid];
    if (tid < tile.t_cnt) sP[tid] = (int)(a.P[tile.p_off + tid] - tile.n_lo);
    auto copy_table = [&](int first, int stride) {
        if (!a.resample) return;
        if (a.interp) {
            const int cnt = a.oversample * (NF + 1);
            for (int i = first; i < cnt; i += stride) tab4[i] = a.tab4[i];
        } else {
            for (int i = first; i < a.sinc_len; i += stride) stab[i] = a.sinc[i];
        }
    };
    // y[n] = (sum_t frame_t[n - P_t]) / (delta[n] + sum_t gain*w[n - P_t]), ascending t, starting from 0.0f
    // (== outputAccumulator / windowAccumulator at the moment writeSlice divides them).  The denominator is
    // data-independent: the host planner evaluates it once per tile with the same float arithmetic
    // (pv_engine.cc build_tiles) and every (stream, channel) row reuses it.  Frames that do not cover n
    // contribute an exact +0.0f (adding +0 never changes a sum that started at +0), so the loads are
    // unconditional on a clamped address: no divergent branch, and the compiler can batch them.
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const bool quads = NR == 2 && nt == 256 && tile.n_cnt <= 4 * 126 && (N & 3) == 0;
    copy_table(tid, nt);
    __syncthreads();
    if (quads) {
        // The gather is bound by the number of load instructions and by their latency: a lane owns four consecutive
        // tile samples and fetches 16 bytes per frame.  A frame starts anywhere, so its samples for those four sit
        // in two neighbouring aligned 16-byte pieces: the lane loads the lower one and takes the upper one from the
        // next lane (DPP wave shift; lane 63 of a wave only serves as its lane 62's neighbour, so a wave covers
        // 63 quads and a pair of waves 126).  Waves 0-1 gather the first row, waves 2-3 the second.
        const int r = wave >> 1;
        const bool row_ok = row0 + r < a.rows;
        const float *__restrict__ fr = a.frames + (int64_t)(row_ok ? row0 + r : row0) * a.FR * N;
        const int u = 63 * (wave & 1) + lane;
        // quads past the tile's last sample are never used (one more serves as the last one's DPP neighbour): they
        // fetch what that neighbour fetches instead of frame data beyond the tile -- the 126 quads of a wave pair
        // cover 504 samples, a tile needs ~400, and the difference was a fifth of the kernel's HBM reads
        const int qmax = (tile.n_cnt + 3) >> 2;
        const int ua = u < qmax ? u : qmax;
        const float4 *__restrict__ fr4 = reinterpret_cast<const float4 *>(fr);
        const int nq = N >> 2;
        const float4 w4 = reinterpret_cast<const float4 *>(wacc)[4 * u < a.lds_floats ? u : 0];
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        constexpr int kF = 4; // frames whose loads are in flight together
        for (int j0 = 0; j0 < tile.t_cnt; j0 += kF) {
            float4 Av[kF];
            int spv[kF];
#pragma unroll
            for (int q = 0; q < kF; ++q) {
                const int j = j0 + q < tile.t_cnt ? j0 + q : tile.t_cnt - 1;
                spv[q] = sP[j];
                const int f0 = 4 * ua - spv[q]; // frame sample under the quad's first tile sample
                const int rr = (-spv[q]) & 3;   // where in its aligned piece that sample sits (wave-uniform)
                const int qf = (f0 - rr) >> 2;
                const int qc = qf < 0 ? 0 : (qf >= nq ? nq - 1 : qf);
                const int slot = (tile.t_first + j) & (a.FR - 1);
                Av[q] = fr4[(int64_t)slot * nq + qc];
            }
#pragma unroll
            for (int q = 0; q < kF; ++q) {
                if (j0 + q >= tile.t_cnt) break; // wave-uniform
                const float4 A = Av[q];
                const int f0 = 4 * u - spv[q];
                const int rr = (-spv[q]) & 3;
                float4 B;
                B.x = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(A.x), 0x130, 0xf, 0xf, false));
                B.y = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(A.y), 0x130, 0xf, 0xf, false));
                B.z = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(A.z), 0x130, 0xf, 0xf, false));
                float v0, v1, v2, v3;
                if (rr == 0) {
                    v0 = A.x, v1 = A.y, v2 = A.z, v3 = A.w;
                } else if (rr == 1) {
                    v0 = A.y, v1 = A.z, v2 = A.w, v3 = B.x;
                } else if (rr == 2) {
                    v0 = A.z, v1 = A.w, v2 = B.x, v3 = B.y;
                } else {
                    v0 = A.w, v1 = B.x, v2 = B.y, v3 = B.z;
                }
                a0 += (f0 >= 0 && f0 < N) ? v0 : 0.f;
                a1 += (f0 + 1 >= 0 && f0 + 1 < N) ? v1 : 0.f;
                a2 += (f0 + 2 >= 0 && f0 + 2 < N) ? v2 : 0.f;
                a3 += (f0 + 3 >= 0 && f0 + 3 < N) ? v3 : 0.f;
            }
        }
        if (lane < 63 && 4 * u < a.lds_floats) {
            const int64_t n0 = tile.n_lo + 4 * u;
            float4 y;
            y.x = n0 >= 0 ? a0 / w4.x : 0.f;
            y.y = n0 + 1 >= 0 ? a1 / w4.y : 0.f;
            y.z = n0 + 2 >= 0 ? a2 / w4.z : 0.f;
            y.w = n0 + 3 >= 0 ? a3 / w4.w : 0.f;
            reinterpret_cast<float4 *>(ola + r * a.lds_floats)[u] = y;
        }
    } else {
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            if (row0 + r >= a.rows) break; // workgroup-uniform
            const float *__restrict__ fr = a.frames + (int64_t)(row0 + r) * a.FR * N;
            for (int i = tid; i < tile.n_cnt; i += nt) {
                float acc = 0.f;
#pragma unroll 4
                for (int j = 0; j < tile.t_cnt; ++j) {
                    const int off = i - sP[j]; // n - P_t
                    const bool in = off >= 0 && off < N;
                    const int slot = (tile.t_first + j) & (a.FR - 1);
                    const float fv = fr[(int64_t)slot * N + (in ? off : 0)];
                    acc += in ? fv : 0.f;
                }
                ola[r * a.lds_floats + i] = tile.n_lo + i >= 0 ? acc / wacc[i] : 0.f;
            }
        }
    }
    __syncthreads();

    if (tid >= tile.kcnt) return;
    const int64_t k = tile.k0 + tid;
    const int nr = a.rows - row0 < NR ? a.rows - row0 : NR; // rows this workgroup really has (>= 1)
    float *__restrict__ out = a.out + (int64_t)row0 * a.out_stride_row + (k - a.k_base);
    if (!a.resample) {
        for (int r = 0; r < nr; ++r) out[(int64_t)r * a.out_stride_row] = ola[r * a.lds_floats + tid];
        return;
    }
    const float *x = ola + (int)(oe.x & 0xffffu); // tap j = 0
    if (a.interp) {
        const int offset = (int)(oe.x >> 16);
        const float frac = __uint_as_float(oe.y);
        const float4 *__restrict__ T = tab4 + offset * (NF + 1);
        v2f a01[NR], a23[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) a01[r] = v2f{0.f, 0.f}, a23[r] = v2f{0.f, 0.f};
#pragma unroll 4
        for (int j = 0; j < NF; ++j) { // NF is a multiple of 4 (resample.c:687)
            const float4 c = T[j];
            const v2f c01 = {c.x, c.y}, c23 = {c.z, c.w};
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const float xv = x[r * a.lds_floats + j]; // a missing second row reads stale LDS: never stored
                const v2f xx = {xv, xv};
                a01[r] += xx * c01; // -ffp-contract=off: separate multiply and add, per element, like the reference
                a23[r] += xx * c23;
            }
        }
        // cubic_coef (resample.c:339-351)
        const float c0 = -0.16667f * frac + 0.16667f * frac * frac * frac;
        const float c1 = frac + 0.5f * frac * frac - 0.5f * frac * frac * frac;
        const float c3 = -0.33333f * frac + 0.5f * frac * frac - 0.16667f * frac * frac * frac;
        const float c2 = (float)(1. - c0 - c1 - c3);
#pragma unroll
        for (int r = 0; r < NR; ++r)
            if (r < nr)
                out[(int64_t)r * a.out_stride_row] = (c0 * a01[r].x) + (c1 * a01[r].y) + (c2 * a23[r].x) + (c3 * a23[r].y);
    } else {
        const float *t = stab + (oe.x >> 16) * (uint32_t)NF;
        for (int r = 0; r < nr; ++r) {
            float sum = 0.f;
            for (int j = 0; j < NF; ++j) sum += x[r * a.lds_floats + j] * t[j];
            out[(int64_t)r * a.out_stride_row] = sum;
        }
    }
}

constexpr int kOlaRows = 2; // rows per workgroup of the batch / streaming overlap-add kernel

template <int kRes> __global__ __launch_bounds__(kTileOut) void pv_ola_kernel(const OlaArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    ola_role<kOlaRows, kRes>(a, blockIdx.x, blockIdx.y * kOlaRows, smem_raw);
}

size_t ola_lds_bytes(const OlaArgs &a, int rows_per_group) {
    return (size_t)a.tab_bytes + sizeof(float) * (size_t)a.lds_floats * rows_per_group + sizeof(int) * kMaxTileFrames;
}

void launch_ola(const OlaArgs &a, hipStream_t st) {
    const size_t lds = ola_lds_bytes(a, kOlaRows);
    const dim3 grid(a.ntiles, (a.rows + kOlaRows - 1) / kOlaRows);
    if (!a.resample) {
        launch_big_lds<pv_ola_kernel<0>>(grid, dim3(kTileOut), lds, st, a);
    } else if (!a.interp) {
        launch_big_lds<pv_ola_kernel<1>>(grid, dim3(kTileOut), lds, st, a);
    } else {
        launch_big_lds<pv_ola_kernel<2>>(grid, dim3(kTileOut), lds, st, a);
    }
}

// --------------------------------------------------------------------------------------------
// Fused synthesis + overlap-add + resample (pv_kernels.h ChainArgs): the reference's streaming state kept in LDS.
//
//   synthesiseSlice (:1057,1073):  outputAccumulator[0..N) += frame         -> acc ring, frame t at P_t
//   writeSlice (:1157-1194):       acc[0..s) /= wacc[0..s); resample or ring-write; shift both by s
//                                  -> finalise [P_t, P_t + s): divide by the host-planned window sum (the
//                                     denominator is data-independent), zero the slots; the normalised samples
//                                     are the output, or go to a small HBM ring for pv_resample_kernel
//
// One workgroup per row; wave w owns slices w, w + W, ...: it synthesises its frame into its LDS region (or takes
// the windowed frame from the HBM frame ring), waits for its turn, adds the frame, finalises and passes the turn on.  Adds happen strictly in slice order, so every accumulator sample sees the
// reference's sequence of float additions; a dropped slice (adv == 0) simply leaves its frame piled where it is.
// There is no workgroup barrier inside the loop: waves drift apart and hide each other's latencies, the turn
// counter only serialises the few hundred cycles of the add.
// --------------------------------------------------------------------------------------------
__device__ __forceinline__ float dpp_ror1(float v) { // lane i <- lane i - 1, lane 0 <- lane 63
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x13C, 0xf, 0xf, false));
}

// ChainArgs::diag is ALWAYS ZERO in the product library: nothing reads AUDIOMOD_PV_CHAIN_DIAG there (pv_engine.cc sets
// the field only under -DPV_DIAG, for tools/chain_diag.sh's elimination runs).  The tests on it stay in the code
// because they are opaque to the compiler: round 3 compiled them out and the kernel ran 20 % SLOWER (0.73 vs 0.60 ms
// per 128 K slices, same source otherwise, profiles/r03/fused_fence_ab.txt) -- without these three conditional
// regions the scheduler moves work across the synthesis / turn / finalise boundaries and pays for it in scalar-register
// reloads.  They are code-motion fences that happen to double as measurement switches in diagnostic builds.
#define PV_CHAIN_DIAG(c, bit) (((c).diag & (bit)) != 0)

struct ChainLds {
    float *acc;   // [AR]
    int *turn;    // next slice whose frame may be added
};
__device__ __forceinline__ ChainLds chain_carve(const ChainArgs &c, char *base) {
    ChainLds l;
    l.acc = reinterpret_cast<float *>(base);
    l.turn = reinterpret_cast<int *>(l.acc + c.AR);
    return l;
}
__host__ __device__ inline size_t chain_shared_bytes(const ChainArgs &c) {
    return sizeof(float) * (size_t)c.AR + 16;
}

// ring images and coefficient table in, before the first slice (whole workgroup)
// (first run of a row: the carried accumulator; later runs start from zeros and rebuild what reaches into their range
// by re-adding the frames before it, ChainSlice flag bit 1)
__device__ __forceinline__ void chain_prologue(const ChainArgs &c, const ChainLds &l, int row, bool first_run = true) {
    const int nt = blockDim.x, tid = threadIdx.x;
    const float4 *sa = reinterpret_cast<const float4 *>(c.st_acc + ((int64_t)(c.acc_sel & 1) * c.rows + row) * c.AR);
    const bool carried = first_run && !(c.acc_sel & 2); // (a stream's first launch starts from the empty accumulator)
    for (int i = tid; i < c.AR / 4; i += nt)
        reinterpret_cast<float4 *>(l.acc)[i] = carried ? sa[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    if (tid == 0) *l.turn = 0;
    __syncthreads();
}
__device__ __forceinline__ void chain_epilogue(const ChainArgs &c, const ChainLds &l, int row, bool last_run = true) {
    __syncthreads(); // every wave has passed its last turn
    if (!last_run) return; // only the run that ends the launch holds the row's true accumulator
    const int nt = blockDim.x, tid = threadIdx.x;
#if defined(PV_DIAG)
    const int wr_half = (c.acc_sel & 4) ? 0 : ((c.acc_sel & 1) ^ 1); // (AUDIOMOD_PV_DEBUG_STALE_ACC: round 2's single buffer)
#else
    const int wr_half = (c.acc_sel & 1) ^ 1;
#endif
    float4 *sa = reinterpret_cast<float4 *>(c.st_acc + ((int64_t)wr_half * c.rows + row) * c.AR);
    for (int i = tid; i < c.AR / 4; i += nt) sa[i] = reinterpret_cast<const float4 *>(l.acc)[i];
}

// What a wave fetches for its slice before it waits for its turn: the first 256 denominators (the rest, for hops
// above 256 samples, are read in the loop).  The output-table entries are fetched after the turn has been passed
// on: inside the turn they would only hold registers.
struct ChainPrefetch {
    float wd[4];
};
__device__ __forceinline__ void chain_prefetch(const ChainArgs &c, const ChainSlice &sl, int row, int lane,
                                               ChainPrefetch &pf) {
    // (the denominators are laid out by ring quads: entry 0 belongs to sample P_t - r)
    const float *__restrict__ wden = ((row % c.C) > 0 ? c.wden_hi : c.wden) + (sl.acc_pos & 3);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int i = lane + 64 * m;
        pf.wd[m] = wden[sl.wden_off + (i < sl.adv ? i : 0)];
    }
}

__device__ __forceinline__ void chain_wait_turn(int *turn, int tl) {
    while (__builtin_amdgcn_readfirstlane(__hip_atomic_load(turn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != tl)
        __builtin_amdgcn_s_sleep(1);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}
__device__ __forceinline__ void chain_pass_turn(int *turn, int tl, int lane) {
    // LDS only: the wave's outstanding global loads and stores are none of the next wave's business
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    if (lane == 0) __hip_atomic_store(turn, tl + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Add NP pieces of a frame (piece j = this lane's four windowed samples 4 (lane + 64 (j0 + j)) .. + 3, zeros past the
// frame's end) into the accumulator ring.  The ring is updated in aligned quads: a frame that starts r = R_ samples
// into a quad is shifted by r through the neighbouring lane (DPP rotate; lane 0 takes lane 63 of the previous
// piece, carried in prevR between calls).  Positions outside the frame receive +0.0f, which leaves any sum that
// started from +0.0f as it is.  `last`: also the quad that holds the frame's final r samples.
template <int R_, int NP>
__device__ __forceinline__ void chain_add_pieces(float *acc, const int AQ, const int a, const int NQ, const int lane,
                                                 const int j0, const float4 (&A)[NP], float4 &prevR, const bool last) {
    float4 *acc4 = reinterpret_cast<float4 *>(acc);
    const int qend = NQ + (R_ ? 1 : 0); // quads the frame touches
    // The quads of a frame are distinct, so every read may be issued before the first write: the add is inside the
    // turn, where a chain of read -> add -> write round trips per quad is time every other wave of the row waits.
    constexpr int NS = NP + (R_ ? 1 : 0);
    float4 V[NS];
    auto quad_of = [&](int j) -> int { // ring quad of this lane's piece j, or -1 when it lies past the frame
        const int u = lane + 64 * (j0 + j);
        int qq = a + u;
        if (qq >= AQ) qq -= AQ;
        return (u < qend && (j < NP || last)) ? qq : -1;
    };
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int qq = quad_of(j);
        V[j] = acc4[qq >= 0 ? qq : 0];
    }
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const float4 Aj = j < NP ? A[j < NP ? j : 0] : make_float4(0.f, 0.f, 0.f, 0.f);
        float4 S = Aj;
        if (R_ != 0) {
            const float4 Rr = make_float4(dpp_ror1(Aj.x), dpp_ror1(Aj.y), dpp_ror1(Aj.z), dpp_ror1(Aj.w));
            const float4 P = lane == 0 ? prevR : Rr;
            if (j < NP) prevR = Rr;
            if (R_ == 1) S = make_float4(P.w, Aj.x, Aj.y, Aj.z);
            else if (R_ == 2) S = make_float4(P.z, P.w, Aj.x, Aj.y);
            else S = make_float4(P.y, P.z, P.w, Aj.x);
        }
        V[j].x += S.x, V[j].y += S.y, V[j].z += S.z, V[j].w += S.w;
    }
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int qq = quad_of(j);
        if (qq >= 0) acc4[qq] = V[j];
    }
}
template <int NP>
__device__ __forceinline__ void chain_add_dispatch(float *acc, int AR, int acc_pos, int NQ, int lane, int j0,
                                                   const float4 (&A)[NP], float4 &prevR, bool last) {
    const int r = acc_pos & 3, AQ = AR >> 2, a = acc_pos >> 2; // r is wave-uniform
    if (r == 0) chain_add_pieces<0, NP>(acc, AQ, a, NQ, lane, j0, A, prevR, last);
    else if (r == 1) chain_add_pieces<1, NP>(acc, AQ, a, NQ, lane, j0, A, prevR, last);
    else if (r == 2) chain_add_pieces<2, NP>(acc, AQ, a, NQ, lane, j0, A, prevR, last);
    else chain_add_pieces<3, NP>(acc, AQ, a, NQ, lane, j0, A, prevR, last);
}

template <int kRes> // 0 = the finalised samples are the output, 1 = they go to the stream ring of the resampler
__device__ __forceinline__ void chain_finish_slice(const ChainArgs &c_in, const ChainLds &l, const ChainSlice &sl,
                                                   const ChainPrefetch &pf, const int row, const int tl, const int lane) {
    ChainArgs c = c_in;
    c.resample = kRes != 0;
    // ---- finalise [P_t, P_t + adv): acc / window sum -> stream ring (or straight out when nothing resamples)
    const float *__restrict__ wden = ((row % c.C) > 0 ? c.wden_hi : c.wden) + (sl.acc_pos & 3);
    float *__restrict__ out = c.out + (int64_t)row * c.out_stride_row + sl.k_off;
    float *__restrict__ stream = c.stream + (int64_t)row * ((int64_t)c.smask + 1);
    auto acc_index = [&](int i) {
        int ai = sl.acc_pos + i;
        return ai >= c.AR ? ai - c.AR : ai;
    };
    const bool quiet = (sl.flags & 2) != 0; // a warm-up slice of a later run: its samples belong to the run before
    auto emit = [&](int i, float y) {
        if (quiet) return;
        if (c.resample) {
            stream[(uint32_t)(sl.str_pos + i) & (uint32_t)c.smask] = y;
        } else if (i < sl.kcnt) {
            out[i] = y;
        }
    };
    if (!PV_CHAIN_DIAG(c, 2)) {
        // (all reads, then the divisions, then the writes: this is still inside the turn)
        float v[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int i = lane + 64 * m;
            v[m] = i < sl.adv ? l.acc[acc_index(i)] : 0.f;
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int i = lane + 64 * m;
            if (i < sl.adv) {
                l.acc[acc_index(i)] = 0.f;
                emit(i, v[m] / pf.wd[m]);
            }
        }
        for (int i = 256 + lane; i < sl.adv; i += 64) {
            const int ai = acc_index(i);
            const float y = l.acc[ai] / wden[sl.wden_off + i];
            l.acc[ai] = 0.f;
            emit(i, y);
        }
    }
    // ---- the next frame may be added now
    chain_pass_turn(l.turn, tl, lane);
}

// The wave-FFT kernel's version of "wait, add, finalise, pass the turn".  Everything that does not need the
// accumulator happens before the wait (the frame shifted to the ring's quad alignment, the denominators fetched),
// and inside the turn a lane reads its quads, adds, and writes them back once -- zeros where a sample belongs to
// [P_t, P_t + adv), which this frame completes (writeSlice's divide + shift, :1157-1194): those sums stay in the
// lane's registers and are normalised and appended to the stream after the turn has been passed on.  The second
// counter publishes, in slice order, that a slice's stream samples are written (the next slice's wave resamples the
// outputs this one deferred).  wden is laid out by ring quads: entry 0 belongs to sample P_t - r.
// (kFast: the denominators arrive as reciprocals -- the host inverts them, pv_engine.cc -- and normalising is a multiply)
template <int R_, int NP, int kRes, bool kFast = false>
__device__ __forceinline__ void chain_slice_tail(const ChainArgs &c_in, const ChainLds &l, const ChainSlice &sl,
                                                 const float4 (&A)[NP], const bool skip, const int row, const int tl,
                                                 const int lane) {
    ChainArgs c = c_in;
    c.resample = kRes != 0;
    constexpr int NS = NP + (R_ ? 1 : 0);
    const int AQ = c.AR >> 2, a = sl.acc_pos >> 2;
    float4 *acc4 = reinterpret_cast<float4 *>(l.acc);
    // ---- before the turn
    float4 S[NS];
    {
        float4 prevR = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const float4 Aj = j < NP ? A[j < NP ? j : 0] : make_float4(0.f, 0.f, 0.f, 0.f);
            S[j] = Aj;
            if (R_ != 0) {
                const float4 Rr = make_float4(dpp_ror1(Aj.x), dpp_ror1(Aj.y), dpp_ror1(Aj.z), dpp_ror1(Aj.w));
                const float4 P = lane == 0 ? prevR : Rr;
                prevR = Rr;
                if (R_ == 1) S[j] = make_float4(P.w, Aj.x, Aj.y, Aj.z);
                else if (R_ == 2) S[j] = make_float4(P.z, P.w, Aj.x, Aj.y);
                else S[j] = make_float4(P.y, P.z, P.w, Aj.x);
            }
        }
    }
    const float *__restrict__ wden = ((row % c.C) > 0 ? c.wden_hi : c.wden) + sl.wden_off;
    const int fin_quads = (sl.adv + R_ + 3) >> 2; // quads that hold samples of the region being finalised
    float4 wd[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int u = lane + 64 * j;
        wd[j] = *reinterpret_cast<const float4 *>(wden + 4 * (u < fin_quads ? u : 0));
    }
    int q[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int qq = a + lane + 64 * j;
        q[j] = qq >= AQ ? qq - AQ : qq;
    }
    const bool tail_lane = lane == 0; // the quad behind the last full piece belongs to one lane
    // What goes back to the ring: the sum, or zero where the sample is inside [0, adv) relative to P_t --
    // as lane masks in scalar registers (no vector registers held across the wait), made before the turn for the
    // two pieces that reach into the region for hops up to 512 - R samples; later pieces test in place.
    constexpr int NM = NS < 2 ? NS : 2;
    unsigned long long zero_at[NM][4];
#pragma unroll
    for (int j = 0; j < NM; ++j) {
        const int s0 = 4 * (lane + 64 * j) - R_;
        zero_at[j][0] = __builtin_amdgcn_ballot_w64(s0 >= 0 && s0 < sl.adv);
        zero_at[j][1] = __builtin_amdgcn_ballot_w64(s0 + 1 >= 0 && s0 + 1 < sl.adv);
        zero_at[j][2] = __builtin_amdgcn_ballot_w64(s0 + 2 >= 0 && s0 + 2 < sl.adv);
        zero_at[j][3] = __builtin_amdgcn_ballot_w64(s0 + 3 < sl.adv);
    }
    auto masked = [](float v, unsigned long long m) -> float { // lanes set in m get +0
        float o;
        asm("v_cndmask_b32_e64 %0, %1, 0, %2 ; pvmask" : "=v"(o) : "v"(v), "s"(m));
        return o;
    };
    auto write_back = [&](int j, const float4 v) -> float4 {
        const int s0 = 4 * (lane + 64 * j) - R_;
        float4 wb = v;
        if (j < NM) {
            wb.x = masked(v.x, zero_at[j < NM ? j : 0][0]);
            wb.y = masked(v.y, zero_at[j < NM ? j : 0][1]);
            wb.z = masked(v.z, zero_at[j < NM ? j : 0][2]);
            wb.w = masked(v.w, zero_at[j < NM ? j : 0][3]);
        } else if (256 * j - R_ < sl.adv) { // wave-uniform: this piece reaches into the region (hops above ~500)
            wb.x = (s0 >= 0 && s0 < sl.adv) ? 0.f : v.x;
            wb.y = (s0 + 1 >= 0 && s0 + 1 < sl.adv) ? 0.f : v.y;
            wb.z = (s0 + 2 >= 0 && s0 + 2 < sl.adv) ? 0.f : v.z;
            wb.w = (s0 + 3 < sl.adv) ? 0.f : v.w;
        }
        return wb;
    };
    // The masks are pinned in their scalar registers HERE, in front of the wait.  Not for speed (measured: pinning the
    // shifted frame as well, so that the compiler cannot sink its selects into the turn, costs 0.320 -> 0.349 ms per
    // launch in spills; addresses and masks only: 0.320; raised priority alone: 0.315) but for correctness: on gfx950 a
    // VALU instruction that reads an SGPR written by a VALU instruction (the v_cmp behind a ballot) needs two wait states
    // in between, the compiler's hazard recogniser inserts them for its own instructions only, and masked() is inline
    // assembly -- left free, the compiler may put the compare right in front of it (seen as a rare wrong write-back:
    // test_fused_overlap_add_is_bit_identical_to_the_tile_path failed once in four full runs).  With the compares
    // forced to this side of the wait loop, the loop's own instructions are the distance.
    // The s_nop inside the pin makes the distance part of the instruction stream rather than a property of what the
    // compiler happens to schedule behind it: every compare that produced a mask is in front of this statement (the
    // masks are its operands), every masked() behind it.
#pragma unroll
    for (int j = 0; j < NM; ++j)
        asm volatile("s_nop 1 ; pvpin" : "+s"(zero_at[j][0]), "+s"(zero_at[j][1]), "+s"(zero_at[j][2]), "+s"(zero_at[j][3]));
    // ---- the turn
    if (!PV_CHAIN_DIAG(c, 4)) chain_wait_turn(l.turn, tl);
    __builtin_amdgcn_s_setprio(3); // the turn's instructions ahead of the three other waves of this SIMD
    float4 V[NS];
    if (!skip) {
#pragma unroll
        for (int j = 0; j < NS; ++j) V[j] = acc4[q[j]];
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            V[j].x += S[j].x, V[j].y += S[j].y, V[j].z += S[j].z, V[j].w += S[j].w;
            if (j < NP || tail_lane) acc4[q[j]] = write_back(j, V[j]);
        }
    } else {
        // a frame this channel does not add (CONSTANT-mode overrun): adv is 0 then, nothing is finalised either and
        // V is never looked at (left undefined rather than zero-filled: 36 moves the common path would execute too)
#pragma unroll
        for (int j = 0; j < NS; ++j) asm volatile("" : "=v"(V[j].x), "=v"(V[j].y), "=v"(V[j].z), "=v"(V[j].w));
    }
    chain_pass_turn(l.turn, tl, lane);
    __builtin_amdgcn_s_setprio(0);
    // ---- after the turn: normalise the finalised samples and append them to the stream (or emit them)
    float *__restrict__ out = c.out + (int64_t)row * c.out_stride_row + sl.k_off;
    float *__restrict__ stream = c.stream + (int64_t)row * ((int64_t)c.smask + 1);
    const bool quiet = (sl.flags & 2) != 0; // a warm-up slice of a later run: its samples belong to the run before
    auto emit = [&](int sidx, float y) { // sidx: sample index relative to P_t
        if (quiet || sidx < 0 || sidx >= sl.adv) return;
        if (c.resample) {
            stream[(uint32_t)(sl.str_pos + sidx) & (uint32_t)c.smask] = y;
        } else if (sidx < sl.kcnt) {
            out[sidx] = y;
        }
    };
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        if (256 * j - R_ < sl.adv) { // wave-uniform
            const int u = lane + 64 * j;
            const float4 d = j < 2 ? wd[j < 2 ? j : 0]
                                   : *reinterpret_cast<const float4 *>(wden + 4 * (u < fin_quads ? u : 0));
            const int s0 = 4 * u - R_;
            if (j < NP || tail_lane) {
                emit(s0, kFast ? V[j].x * d.x : V[j].x / d.x);
                emit(s0 + 1, kFast ? V[j].y * d.y : V[j].y / d.y);
                emit(s0 + 2, kFast ? V[j].z * d.z : V[j].z / d.z);
                emit(s0 + 3, kFast ? V[j].w * d.w : V[j].w / d.w);
            }
        }
    }
}

// (the all-modes variant -- frequency compression, vocoder, ... -- needs ~150 VGPRs where the plain ones fit 128:
// compiled for twelve waves per workgroup, three per SIMD, instead of spilling)
// Threads per workgroup each variant is compiled for: sixteen waves (128 registers) for the specialisations, twelve for
// the all-modes kernel and the exact formant / gender one (~150 registers); the free-form formant / gender kernel fits
// 128 (round 3).  4096-point frames: eight waves (LDS).  Core::init sizes the launch by the same rule.
constexpr int chain_kernel_max_threads(int NC, int kPlainCore, bool kFast) {
    return NC <= 1024 ? ((kPlainCore < 0 || (kPlainCore == 3 && !kFast)) ? 768 : 1024) : 512;
}
template <int NC, int kPlainCore, int kRes, bool kFast = false>
__global__ __launch_bounds__(chain_kernel_max_threads(NC, kPlainCore, kFast)) void pv_synth_chain_kernel(
    const SynthArgs s, const ChainArgs c) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    using W = WF<NC>;
    constexpr int N = 2 * NC, hs = NC, NQ = N / 4, NP = NQ / 64;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int row = blockIdx.x, run = blockIdx.y;
    // a row's slices of the launch are split into gridDim.y runs, one workgroup each (entry i of a run's list is its
    // i-th slice in order, warm-up slices first; ChainSlice::tl says which slice of the launch it is)
    const int i_begin = c.run_off[run], i_count = c.run_off[run + 1] - i_begin;
    cf *wlds = reinterpret_cast<cf *>(smem_raw) + wave * W::LDS_CF;
    const ChainLds l = chain_carve(c, smem_raw + (size_t)c.waves * W::LDS_CF * sizeof(cf));
    chain_prologue(c, l, row, run == 0);
    const float *__restrict__ w = s.tb.window;
    const bool upper = (row % c.C) > 0;
    const int lane0 = lane;
    for (int i = wave; i < i_count; i += c.waves) {
        // the lane id, made opaque once per iteration: everything derived from it is recomputed per slice instead of
        // being hoisted out of the loop and held in registers (which spilled ~100 VGPRs)
        int lane = lane0;
        asm volatile("" : "+v"(lane));
        const ChainSlice sl = c.slices[i_begin + i];
        const int tl = sl.tl;
        const bool skip = (sl.flags & 1) && upper; // wave-uniform
        float4 A[NP];
        if (!skip) {
            if (!PV_CHAIN_DIAG(c, 8)) synth_wave_role<NC, kPlainCore, 1, kFast>(s, row, tl, wlds, lane);
            // ifftshift + synthesis window (phasevocoderimpl.h:183-198): four consecutive samples per lane and piece
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                const int i = 4 * (lane + 64 * j);
                const int e = ((i + hs) & (N - 1)) >> 1;
                const cf z0 = wlds[W::pad(e)], z1 = wlds[W::pad(e) + 1];
                const float4 ww = *reinterpret_cast<const float4 *>(w + i);
                A[j] = make_float4(z0.x * ww.x, z0.y * ww.y, z1.x * ww.z, z1.y * ww.w);
            }
        }
        const int r = sl.acc_pos & 3; // wave-uniform
        if (r == 0) chain_slice_tail<0, NP, kRes, kFast>(c, l, sl, A, skip, row, i, lane);
        else if (r == 1) chain_slice_tail<1, NP, kRes, kFast>(c, l, sl, A, skip, row, i, lane);
        else if (r == 2) chain_slice_tail<2, NP, kRes, kFast>(c, l, sl, A, skip, row, i, lane);
        else chain_slice_tail<3, NP, kRes, kFast>(c, l, sl, A, skip, row, i, lane);
    }
    chain_epilogue(c, l, row, run == (int)gridDim.y - 1);
}

// Any FFT size: the synthesis kernel has written the windowed frames to the HBM frame ring; the chain takes them
// from there, up to eight pieces (2048 samples) at a time.
template <int kRes> __global__ __launch_bounds__(1024) void pv_frames_chain_kernel(const ChainArgs c) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int row = blockIdx.x, run = blockIdx.y;
    const int i_begin = c.run_off[run], i_count = c.run_off[run + 1] - i_begin;
    const ChainLds l = chain_carve(c, smem_raw);
    chain_prologue(c, l, row, run == 0);
    const int NQ = c.N >> 2;
    const int groups = (NQ + 511) >> 9;
    const bool upper = (row % c.C) > 0;
    for (int i = wave; i < i_count; i += c.waves) {
        const ChainSlice sl = c.slices[i_begin + i];
        const int tl = sl.tl;
        const bool skip = (sl.flags & 1) && upper;
        ChainPrefetch pf;
        chain_prefetch(c, sl, row, lane, pf);
        const int fslot = (int)((c.t0 + tl) & (int64_t)(c.FR - 1));
        const float4 *__restrict__ fr =
            reinterpret_cast<const float4 *>(c.frames + ((int64_t)row * c.FR + fslot) * c.N);
        auto load_group = [&](int g, float4 (&A)[8]) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int u = lane + 64 * (8 * g + j);
                A[j] = (u < NQ && !skip) ? fr[u] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        };
        float4 A[8];
        load_group(0, A);
        chain_wait_turn(l.turn, i);
        if (!skip) {
            float4 prevR = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int g = 0; g < groups; ++g) {
                if (g > 0) load_group(g, A);
                chain_add_dispatch<8>(l.acc, c.AR, sl.acc_pos, NQ, lane, 8 * g, A, prevR, g == groups - 1);
            }
            wave_sync();
        }
        chain_finish_slice<kRes>(c, l, sl, pf, row, i, lane);
    }
    chain_epilogue(c, l, row, run == (int)gridDim.y - 1);
}

size_t chain_lds_bytes(const ChainArgs &a, int nc_wave) {
    const size_t per_wave = nc_wave == 256    ? WF<256>::LDS_CF * sizeof(cf)
                            : nc_wave == 512  ? WF<512>::LDS_CF * sizeof(cf)
                            : nc_wave == 1024 ? WF<1024>::LDS_CF * sizeof(cf)
                            : nc_wave == 2048 ? WF<2048>::LDS_CF * sizeof(cf) : 0;
    return (size_t)a.waves * per_wave + chain_shared_bytes(a);
}

// --- Where a fused kernel is chosen (all four sets: this batch kernel and the pool / pmix / mb slot-table kernels) ---
static bool chain_nc_has_wave(int nc) { return nc == 256 || nc == 512 || nc == 1024 || nc == 2048; }

// Diagnostics: the census of the launchers' choices (pv_kernels.h).  Fixed tables of relaxed atomic counters: a launch
// with the census off tests g_census_on and nothing else; with it on it adds one to one counter (no lock, no
// allocation either way).
static std::atomic<bool> g_census_on{false};
static constexpr int kCensusNc = 4, kCensusCore = 5; // NC 256 ... 2048; kPlainCore -1 ... 3
static std::atomic<uint64_t> g_census_chain[PV_CENSUS_SETS][kCensusNc][kCensusCore][2][2];
static std::atomic<uint64_t> g_census_res[PV_CENSUS_SETS][2][2];
static std::atomic<uint64_t> g_census_rrung[PV_CENSUS_SETS][kResRungs][2][2];
static std::atomic<uint64_t> g_census_ana[PV_CENSUS_SETS][kCensusNc][2];
static std::atomic<uint64_t> g_census_phase[PV_CENSUS_SETS][kPhaseForms][4];
static std::atomic<uint64_t> g_census_akern[PV_CENSUS_SETS][kAnaKernels][6];
static std::atomic<uint64_t> g_census_cep[PV_CENSUS_SETS][kCepKernels][6];
static std::atomic<uint64_t> g_census_voice[PV_CENSUS_SETS][6];
static int census_akern_nc_index(int nc) { // fft / 2 of 256 ... 8192 points
    return nc == 128 ? 0 : nc == 256 ? 1 : nc == 512 ? 2 : nc == 1024 ? 3 : nc == 2048 ? 4 : nc == 4096 ? 5 : -1;
}
static int census_phase_index(int b) { return b == 1 ? 0 : b == 3 ? 1 : b == 4 ? 2 : b == 8 ? 3 : -1; }
static int census_nc_index(int nc) { return nc == 256 ? 0 : nc == 512 ? 1 : nc == 1024 ? 2 : nc == 2048 ? 3 : -1; }
static inline void census_chain(int set, int nc, int plain_core, int res, bool fast) {
    if (!g_census_on.load(std::memory_order_relaxed)) return;
    g_census_chain[set][census_nc_index(nc)][plain_core + 1][res][fast ? 1 : 0].fetch_add(1, std::memory_order_relaxed);
}
static inline void census_resample(int set, bool fast, bool interp) {
    if (!g_census_on.load(std::memory_order_relaxed)) return;
    g_census_res[set][fast ? 1 : 0][interp ? 1 : 0].fetch_add(1, std::memory_order_relaxed);
}
static inline void census_resample_rung(int set, int rung, bool interp, size_t lds) {
    if (!g_census_on.load(std::memory_order_relaxed)) return;
    g_census_rrung[set][rung][interp ? 1 : 0][lds > 64 * 1024 ? 1 : 0].fetch_add(1, std::memory_order_relaxed);
}
static inline void census_analyze(int set, int nc, bool split) {
    if (!g_census_on.load(std::memory_order_relaxed)) return;
    g_census_ana[set][census_nc_index(nc)][split ? 1 : 0].fetch_add(1, std::memory_order_relaxed);
}
static void census_phase(int set, int form, int b) {
    if (!g_census_on.load(std::memory_order_relaxed)) return;
    g_census_phase[set][form][census_phase_index(b)].fetch_add(1, std::memory_order_relaxed);
}
static void census_analysis_kernel(int set, int kernel, int nc) {
    if (!g_census_on.load(std::memory_order_relaxed)) return;
    if (census_akern_nc_index(nc) >= 0) g_census_akern[set][kernel][census_akern_nc_index(nc)].fetch_add(1, std::memory_order_relaxed);
}
static void census_cepstral(int set, int kernel, int nc) {
    if (!g_census_on.load(std::memory_order_relaxed)) return;
    if (census_akern_nc_index(nc) >= 0) g_census_cep[set][kernel][census_akern_nc_index(nc)].fetch_add(1, std::memory_order_relaxed);
}
void census_voice(int set, int nc) { // (pv_whisper.hip launch_whisper)
    if (!g_census_on.load(std::memory_order_relaxed)) return;
    if (census_akern_nc_index(nc) >= 0) g_census_voice[set][census_akern_nc_index(nc)].fetch_add(1, std::memory_order_relaxed);
}
void chain_census_enable(bool on) {
    g_census_on.store(false, std::memory_order_relaxed);
    for (auto &a : g_census_chain) for (auto &b : a) for (auto &c : b) for (auto &d : c) for (auto &e : d) e.store(0, std::memory_order_relaxed);
    for (auto &a : g_census_res) for (auto &b : a) for (auto &c : b) c.store(0, std::memory_order_relaxed);
    for (auto &a : g_census_rrung) for (auto &b : a) for (auto &c : b) for (auto &d : c) d.store(0, std::memory_order_relaxed);
    for (auto &a : g_census_ana) for (auto &b : a) for (auto &c : b) c.store(0, std::memory_order_relaxed);
    for (auto &a : g_census_phase) for (auto &b : a) for (auto &c : b) c.store(0, std::memory_order_relaxed);
    for (auto &a : g_census_akern) for (auto &b : a) for (auto &c : b) c.store(0, std::memory_order_relaxed);
    for (auto &a : g_census_cep) for (auto &b : a) for (auto &c : b) c.store(0, std::memory_order_relaxed);
    for (auto &a : g_census_voice) for (auto &b : a) b.store(0, std::memory_order_relaxed);
    g_census_on.store(on, std::memory_order_relaxed);
}
int64_t chain_census_count(int kind, int set, int a, int b, int c, int d) {
    if (set < 0 || set >= PV_CENSUS_SETS) return -1;
    const auto flag = [](int v) { return v == 0 || v == 1; };
    switch (kind) {
    case 0:
        if (census_nc_index(a) < 0 || b < -1 || b > 3 || !flag(c) || !flag(d)) return -1;
        return (int64_t)g_census_chain[set][census_nc_index(a)][b + 1][c][d].load(std::memory_order_relaxed);
    case 1:
        if (!flag(a) || !flag(b)) return -1;
        return (int64_t)g_census_res[set][a][b].load(std::memory_order_relaxed);
    case 2:
        if (census_nc_index(a) < 0 || !flag(b)) return -1;
        return (int64_t)g_census_ana[set][census_nc_index(a)][b].load(std::memory_order_relaxed);
    case 3:
        if (a < 0 || a >= kPhaseForms || census_phase_index(b) < 0) return -1;
        return (int64_t)g_census_phase[set][a][census_phase_index(b)].load(std::memory_order_relaxed);
    case 4:
        if (a < 0 || a >= kResRungs || !flag(b) || !flag(c)) return -1;
        return (int64_t)g_census_rrung[set][a][b][c].load(std::memory_order_relaxed);
    case 5:
        if (a < 0 || a >= kAnaKernels || census_akern_nc_index(b) < 0) return -1;
        return (int64_t)g_census_akern[set][a][census_akern_nc_index(b)].load(std::memory_order_relaxed);
    case 7: // (PV_CENSUS_CEPSTRAL; 6 is no kind)
        if (a < 0 || a >= kCepKernels || census_akern_nc_index(b) < 0) return -1;
        return (int64_t)g_census_cep[set][a][census_akern_nc_index(b)].load(std::memory_order_relaxed);
    case 8: // (PV_CENSUS_VOICE)
        if (census_akern_nc_index(a) < 0) return -1;
        return (int64_t)g_census_voice[set][census_akern_nc_index(a)].load(std::memory_order_relaxed);
    default: return -1;
    }
}

// The specialisation (kPlainCore) a configuration gets: 0 / 1 / 2 = the plain kernel of that core mode, 3 = frequency
// compensation with the phase-locked core (formant / gender modes; nc 1024, that is fft 2048, only), -1 = the all-modes kernel.
int synth_chain_plain_core(const SynthArgs &s) {
    const bool plain = !s.do_freq_comp && s.voc_band_len < 0 && !s.robotic && !s.passthru && !s.whisper &&
                       !synth_generic_only() && s.coremode >= 0 && s.coremode <= 2;
    const bool fc_locked = s.do_freq_comp && s.voc_band_len < 0 && !s.robotic && !s.passthru && !s.whisper &&
                           !synth_generic_only() && s.coremode == 1;
    if (fc_locked) return s.tb.nc == 1024 ? 3 : -1;
    return plain ? s.coremode : -1;
}
// does launch_synth_chain pick a free-form kernel for this configuration?  (the engine then uploads the window-sum
// denominators as reciprocals)
bool synth_chain_has_fast(const SynthArgs &s) { return chain_nc_has_wave(s.tb.nc) && synth_chain_plain_core(s) >= 0; }

// The ladder from run-time values to template arguments, in three steps: nc -> NC, the predicate's value -> kPlainCore,
// (c.resample, c.fast) -> (kRes, kFast).  A new size or specialisation is added here, once.  What differs between the
// kernel sets is in `Set` (BatchChainSet below, PoolChainSet, PmixChainSet, MbChainSet further down):
//   set.launch<NC, kPlainCore, kRes, kFast>(c, block, lds)   names the kernel, its grid and trailing arguments;
//   Set::max_threads(NC, kPlainCore, kFast)                  the launch bounds the kernel is compiled for;
//   Set::fit_waves(c, max_threads)                           what a launch wider than that does (false: no launch).
// launch == false: the checks only.
// (only the specialisations have a free-form twin: an all-modes launch is kFast = false whatever c.fast says)
static constexpr bool chain_uses_fast(int plain_core, bool fast) { return plain_core >= 0 && fast; }
int synth_chain_max_waves(const SynthArgs &s, bool fast) {
    const int plain_core = synth_chain_plain_core(s);
    if (!chain_nc_has_wave(s.tb.nc)) return plain_core >= 0 ? 16 : 12;
    return chain_kernel_max_threads(s.tb.nc, plain_core, chain_uses_fast(plain_core, fast)) / 64;
}
template <class Set, int NC, int kPlainCore> static bool launch_chain_variant(const Set &set, const ChainArgs &c_in, bool launch) {
    const bool use_fast = chain_uses_fast(kPlainCore, c_in.fast);
    const int max_threads = use_fast ? Set::max_threads(NC, kPlainCore, true) : Set::max_threads(NC, kPlainCore, false);
    ChainArgs c = c_in;
    if (!Set::fit_waves(c, max_threads)) return false;
    const size_t lds = chain_lds_bytes(c, NC);
    if (!launch) return true;
    census_chain(Set::census_set, NC, kPlainCore, c.resample ? 1 : 0, use_fast);
    const dim3 block(64 * c.waves);
    if constexpr (kPlainCore >= 0) { // the specialisations have a free-form (PV_ARITH_FAST) twin
        if (c.fast) {
            if (!c.resample) set.template launch<NC, kPlainCore, 0, true>(c, block, lds);
            else set.template launch<NC, kPlainCore, 1, true>(c, block, lds);
            return true;
        }
    }
    if (!c.resample) set.template launch<NC, kPlainCore, 0, false>(c, block, lds);
    else set.template launch<NC, kPlainCore, 1, false>(c, block, lds);
    return true;
}
template <class Set, int NC> static bool launch_chain_core(const Set &set, const ChainArgs &c, int plain_core, bool launch) {
    if constexpr (NC == 1024) // the only size with the frequency-compensation specialisation
        if (plain_core == 3) return launch_chain_variant<Set, NC, 3>(set, c, launch);
    switch (plain_core) {
    case 1: return launch_chain_variant<Set, NC, 1>(set, c, launch);
    case 0: return launch_chain_variant<Set, NC, 0>(set, c, launch);
    case 2: return launch_chain_variant<Set, NC, 2>(set, c, launch);
    default: return launch_chain_variant<Set, NC, -1>(set, c, launch);
    }
}
// (nc: the wave transform's size; false where there is none)
template <class Set> static bool launch_chain(const Set &set, const SynthArgs &s, int nc, const ChainArgs &c, bool launch) {
    const int plain_core = synth_chain_plain_core(s);
    switch (nc) {
    case 256: return launch_chain_core<Set, 256>(set, c, plain_core, launch);   // fft 512
    case 512: return launch_chain_core<Set, 512>(set, c, plain_core, launch);   // fft 1024
    case 1024: return launch_chain_core<Set, 1024>(set, c, plain_core, launch); // fft 2048
    case 2048: return launch_chain_core<Set, 2048>(set, c, plain_core, launch); // fft 4096
    default: return false;
    }
}

struct BatchChainSet { // grid (rows, runs); no trailing arguments
    static constexpr int census_set = 0;
    const SynthArgs &s;
    hipStream_t st;
    static constexpr int max_threads(int NC, int kPlainCore, bool kFast) { return chain_kernel_max_threads(NC, kPlainCore, kFast); }
    static bool fit_waves(const ChainArgs &c, int max_threads) {
        if (64 * c.waves <= max_threads) return true;
        // (never: Core::init sizes chain_waves by the same rule; a launch beyond the bounds faults)
        fprintf(stderr, "audiomod_pv: fused kernel launch of %d waves exceeds its bounds (%d threads): not launched\n", c.waves, max_threads);
        return false;
    }
    template <int NC, int kPlainCore, int kRes, bool kFast> void launch(const ChainArgs &c, dim3 block, size_t lds) const {
        launch_big_lds<pv_synth_chain_kernel<NC, kPlainCore, kRes, kFast>>(dim3(c.rows, c.runs), block, lds, st, s, c);
    }
};
void launch_synth_chain(const SynthArgs &s, const ChainArgs &c, hipStream_t st) {
    // (the engine comes here for the four sizes with a wave transform only; any other would get the 4096-point
    // kernel, as it always did)
    (void)launch_chain(BatchChainSet{s, st}, s, chain_nc_has_wave(s.tb.nc) ? s.tb.nc : 2048, c, true);
}

void launch_frames_chain(const ChainArgs &c, hipStream_t st) {
    const size_t lds = chain_lds_bytes(c, 0);
    const dim3 grid(c.rows, c.runs), block(64 * c.waves);
    if (!c.resample) {
        launch_big_lds<pv_frames_chain_kernel<0>>(grid, block, lds, st, c);
    } else {
        launch_big_lds<pv_frames_chain_kernel<1>>(grid, block, lds, st, c);
    }
}

// --------------------------------------------------------------------------------------------
// Speex resampling of the normalised overlap-add stream (the fused path's second kernel): a tile of 256 outputs of
// two rows; the samples its windows cover are one contiguous run of each row's stream ring, copied to LDS, then every
// thread runs resampler_basic_interpolate_single / resampler_basic_direct_single (speex/resample.c:462-560, 353-401)
// for the same output of both rows, so that a tap's coefficients are read once for two outputs (all rows share one
// schedule).  Separate multiply and add (-ffp-contract=off), tap order and accumulators as in the reference.
// --------------------------------------------------------------------------------------------
constexpr int kResRows = 4; // rows per workgroup of the resampling kernel: a tap's coefficients are read once for all

template <int kRes> // 1 = direct sinc table, 2 = cubic-interpolated table
__global__ __launch_bounds__(kTileOut) void pv_resample_kernel(const ResArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    constexpr int NR = kResRows;
    float4 *tab4 = reinterpret_cast<float4 *>(smem_raw);
    float *stab = reinterpret_cast<float *>(smem_raw);
    float *xs = reinterpret_cast<float *>(smem_raw + a.tab_bytes); // [NR][lds_floats]
    const int nt = blockDim.x, tid = threadIdx.x;
    const ResTile tile = a.tiles[blockIdx.x];
    const int row0 = blockIdx.y * NR, NF = a.filt_len;
    const int nr = a.rows - row0 < NR ? a.rows - row0 : NR;
    uint2 oe = make_uint2(0u, 0u);
    if (tid < tile.kcnt) oe = a.otab[(int64_t)blockIdx.x * kTileOut + tid];
    // the tile's stream samples of every row, all loads in flight before the first LDS write (a tile needs at most
    // two samples per thread and row at the ratios that resample: n_cnt <= 256 * num/den + filt_len)
    float xv[NR][2];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const float *__restrict__ st = a.stream + (int64_t)(r < nr ? row0 + r : row0) * ((int64_t)a.smask + 1);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int i = tid + h * kTileOut;
            const int64_t n = tile.n_lo + i; // the stream is zero before its first sample (skip_zeros, :1225)
            xv[r][h] = (i < tile.n_cnt && n >= 0) ? st[(uint32_t)n & (uint32_t)a.smask] : 0.f;
        }
    }
    if (kRes == 2) {
        const int cnt = a.oversample * (NF + 1);
        for (int i = tid; i < cnt; i += nt) tab4[i] = a.tab4[i];
    } else {
        for (int i = tid; i < a.sinc_len; i += nt) stab[i] = a.sinc[i];
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int i = tid + h * kTileOut;
            if (i < tile.n_cnt) xs[r * a.lds_floats + i] = xv[r][h];
        }
    }
    // (longer tiles -- strong down-sampling, more than two samples per thread -- take the rest in a loop)
    for (int i = tid + 2 * kTileOut; i < tile.n_cnt; i += nt)
        for (int r = 0; r < nr; ++r) {
            const int64_t n = tile.n_lo + i;
            const float *__restrict__ st = a.stream + (int64_t)(row0 + r) * ((int64_t)a.smask + 1);
            xs[r * a.lds_floats + i] = n >= 0 ? st[(uint32_t)n & (uint32_t)a.smask] : 0.f;
        }
    __syncthreads();
    if (tid >= tile.kcnt) return;
    float *__restrict__ out = a.out + (int64_t)row0 * a.out_stride_row + (tile.k0 - a.k_base) + tid;
    const float *x = xs + (int)(oe.x & 0xffffu); // tap j = 0
    if (kRes == 2) {
        const float frac = __uint_as_float(oe.y);
        const float4 *__restrict__ T = tab4 + (int)(oe.x >> 16) * (NF + 1);
        v2f a01[NR], a23[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) a01[r] = v2f{0.f, 0.f}, a23[r] = v2f{0.f, 0.f};
#pragma unroll 4
        for (int j = 0; j < NF; ++j) { // NF is a multiple of 4 (resample.c:687)
            const float4 c = T[j];
            const v2f c01 = {c.x, c.y}, c23 = {c.z, c.w};
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const float xr = x[r * a.lds_floats + j]; // a missing row holds zeros: computed, never stored
                const v2f xx = {xr, xr};
                a01[r] += xx * c01;
                a23[r] += xx * c23;
            }
        }
        // cubic_coef (resample.c:339-351)
        const float c0 = -0.16667f * frac + 0.16667f * frac * frac * frac;
        const float c1 = frac + 0.5f * frac * frac - 0.5f * frac * frac * frac;
        const float c3 = -0.33333f * frac + 0.5f * frac * frac - 0.16667f * frac * frac * frac;
        const float c2 = (float)(1. - c0 - c1 - c3);
#pragma unroll
        for (int r = 0; r < NR; ++r)
            if (r < nr)
                out[(int64_t)r * a.out_stride_row] = (c0 * a01[r].x) + (c1 * a01[r].y) + (c2 * a23[r].x) + (c3 * a23[r].y);
    } else {
        const float *t = stab + (oe.x >> 16) * (uint32_t)NF;
        for (int r = 0; r < nr; ++r) {
            float sum = 0.f;
            for (int j = 0; j < NF; ++j) sum += x[r * a.lds_floats + j] * t[j];
            out[(int64_t)r * a.out_stride_row] = sum;
        }
    }
}

// --------------------------------------------------------------------------------------------
// The same resampling with the arithmetic the 1e-4 RMS contract leaves free (ResArgs::fast; the batch engine's
// default, audiomod_pv.h pv_set_arithmetic).  The output of the reference's interpolating resampler is
//     sum_j x[j] * (c0 T0[j] + c1 T1[j] + c2 T2[j] + c3 T3[j])          (resample.c:494-543, regrouped)
// and the bracket -- the cubic-interpolated filter tap -- depends on the output index only, not on the row: every
// row of a batch follows one schedule.  So a thread interpolates each tap ONCE (one multiply + three fma) and applies
// it to the same output of NR rows with one fma per row: (4 + NR) / NR fused operations per row and tap where the
// reference's operation order needs four multiplies and four adds (~4.5x fewer vector instructions at NR = 8).  The
// result differs from the reference's by rounding only (~1e-7 relative: one accumulator instead of four, fma).
// --------------------------------------------------------------------------------------------
constexpr int kResFastRows = 16; // (8 where the batch has fewer rows or the tile does not fit 64 KB of LDS)

// cubic_coef (resample.c:339-351)
__device__ __forceinline__ float4 res_cubic_coef(const float frac) {
    const float c0 = -0.16667f * frac + 0.16667f * frac * frac * frac;
    const float c1 = frac + 0.5f * frac * frac - 0.5f * frac * frac * frac;
    const float c3 = -0.33333f * frac + 0.5f * frac * frac - 0.16667f * frac * frac * frac;
    const float c2 = (float)(1. - c0 - c1 - c3);
    return make_float4(c0, c1, c2, c3);
}
// the filter tap j of an output whose cubic weights are c, from the four interpolation-table values T[j]
__device__ __forceinline__ float res_cubic_tap(const float4 c, const float4 t) {
    return __builtin_fmaf(c.w, t.w, __builtin_fmaf(c.z, t.z, __builtin_fmaf(c.y, t.y, c.x * t.x)));
}

// One output of NR rows on the vector ALU: the thread's output oe, its group's staged samples xs (row r at r * xstride;
// rows at or past nrl are not staged and read row 0 instead: computed, never stored) and the tables in LDS, stored to
// the first nr rows at out (the output in the group's first row).  pv_resample_fast_kernel's body, and the matrix-core
// kernel's for a workgroup whose samples are not all finite.
template <int kRes, int NR>
__device__ __forceinline__ void res_fast_valu(const ResArgs &a, const uint2 oe, const float *xs, const int xstride,
                                              const int nrl, const float4 *tab4, const float *stab,
                                              float *__restrict__ out, const int nr) {
    const int NF = a.filt_len;
    const float *x = xs + (int)(oe.x & 0xffffu); // tap j = 0
    float acc[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = 0.f;
    if (kRes == 2) {
        const float frac = __uint_as_float(oe.y);
        const float4 cw = res_cubic_coef(frac);
        const float4 *__restrict__ T = tab4 + (int)(oe.x >> 16) * (NF + 1);
#pragma unroll 4
        for (int j = 0; j < NF; ++j) { // NF is a multiple of 4 (resample.c:687)
            // (PV_EXP_RES: elimination builds for timing only -- bit 0 no sample reads, bit 1 no coefficient reads)
#if defined(PV_EXP_RES) && (PV_EXP_RES & 2)
            const float4 c = make_float4(frac, cw.x, cw.y, (float)j);
#else
            const float4 c = T[j];
#endif
            const float h = res_cubic_tap(cw, c);
#pragma unroll
            for (int r = 0; r < NR; ++r) {
#if defined(PV_EXP_RES) && (PV_EXP_RES & 1)
                acc[r] = __builtin_fmaf(frac + (float)r, h, acc[r]);
#else
                acc[r] = __builtin_fmaf(x[(r < nrl ? r : 0) * xstride + j], h, acc[r]);
#endif
            }
        }
    } else {
        const float *t = stab + (oe.x >> 16) * (uint32_t)NF;
#pragma unroll 4
        for (int j = 0; j < NF; ++j) {
            const float h = t[j];
#pragma unroll
            for (int r = 0; r < NR; ++r) acc[r] = __builtin_fmaf(x[(r < nrl ? r : 0) * xstride + j], h, acc[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < NR; ++r)
        if (r < nr) out[(int64_t)r * a.out_stride_row] = acc[r];
}

template <int kRes, int NR> // 1 = direct sinc table, 2 = cubic-interpolated table
__global__ __launch_bounds__(kTileOut) void pv_resample_fast_kernel(const ResArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    float4 *tab4 = reinterpret_cast<float4 *>(smem_raw);
    float *stab = reinterpret_cast<float *>(smem_raw);
    float *xs = reinterpret_cast<float *>(smem_raw + a.tab_bytes); // [NR][lds_floats]
    const int nt = blockDim.x, tid = threadIdx.x;
    const ResTile tile = a.tiles[blockIdx.x];
    const int row0 = blockIdx.y * NR, NF = a.filt_len;
    const int nr = a.rows - row0 < NR ? a.rows - row0 : NR;
    uint2 oe = make_uint2(0u, 0u);
    if (tid < tile.kcnt) oe = a.otab[(int64_t)blockIdx.x * kTileOut + tid];
    // the tile's stream samples of every row (a missing row re-reads the group's first: computed, never stored)
    for (int i = tid; i < tile.n_cnt; i += nt) {
        const int64_t n = tile.n_lo + i; // the stream is zero before its first sample (skip_zeros, :1225)
        float xv[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const float *__restrict__ st = a.stream + (int64_t)(r < nr ? row0 + r : row0) * ((int64_t)a.smask + 1);
            xv[r] = n >= 0 ? st[(uint32_t)n & (uint32_t)a.smask] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) xs[r * a.lds_floats + i] = xv[r];
    }
    if (kRes == 2) {
        const int cnt = a.oversample * (NF + 1);
        for (int i = tid; i < cnt; i += nt) tab4[i] = a.tab4[i];
    } else {
        for (int i = tid; i < a.sinc_len; i += nt) stab[i] = a.sinc[i];
    }
    __syncthreads();
    if (tid >= tile.kcnt) return;
    float *__restrict__ out = a.out + (int64_t)row0 * a.out_stride_row + (tile.k0 - a.k_base) + tid;
    res_fast_valu<kRes, NR>(a, oe, xs, a.lds_floats, NR, tab4, stab, out, nr);
}

// --------------------------------------------------------------------------------------------
// The same outputs on the f32 matrix cores (the default; AUDIOMOD_PV_RES_MFMA=0 selects pv_resample_fast_kernel).
// All rows follow one schedule, so 16 consecutive outputs n0 .. n0+15 of a tile and the 16 rows of a workgroup are a
// small banded product
//     Out[r][n] = sum_t X[r][t] B[t][n],   B[t][n] = h_n(t - off_n) for 0 <= t - off_n < NF, else 0,
// t running from off_n0 over ceil((off_n15 - off_n0 + NF) / 4) K-steps of v_mfma_f32_16x16x4_f32: lane l holds the
// sample X[row l&15][t + (l>>4)] (one ds_read_b32) and the tap B[t + (l>>4)][n0 + (l&15)], interpolated exactly as
// res_fast_valu does.  That instruction is bit for bit a k-ordered chain of f32 fma, so every output sees its taps
// j = 0 .. NF-1 in order, as in the vector loop; the products outside the band are fma(x, 0, acc) = acc for finite x
// (before the band acc is +0, as the loop starts).  So the outputs are the vector kernel's, bit for bit; the samples
// stay in registers for all 16 outputs instead of being re-read from LDS for every tap.
// - Each wave takes four 16-output blocks of its tile, all at once: four independent accumulators (the instruction's
//   dependent latency is 40 cycles against a 32-cycle issue; two blocks at a time measured 0.147 against 0.132 ms per
//   launch).  They run the largest K-step count of the four; a shorter block's extra steps have zero taps and read
//   clamped sample positions.  Capped at 128 registers: four waves per SIMD, what the LDS allows anyway.
// - The K-span is rounded up to a multiple of 4: the staging writes zeros to the four positions past the tile's samples.
// - Row stride xstride = 2 mod 4 floats: the 16 rows x 4 t of an A read fall on distinct banks.  With the flag words it
//   stays within the 16 rows x lds_floats of the vector kernel (the engines size lds_floats >= n_cnt + 7).
// - inf or NaN among the samples would leak into outputs whose band does not cover it (inf * 0 = NaN), so the staging
//   ORs a not-finite flag over them, and a workgroup that sees one runs res_fast_valu instead.
// --------------------------------------------------------------------------------------------
constexpr int kResMfmaRows = 16; // the M of v_mfma_f32_16x16x4_f32: one row group per workgroup
constexpr int kResMfmaBlocks = 4; // 16-output blocks in flight per wave (all four of its blocks)

typedef float v4f __attribute__((ext_vector_type(4)));

__host__ __device__ constexpr int res_mfma_xstride(const int lds_floats) { return ((lds_floats - 2) & ~3) + 2; }

template <int kRes> // 1 = direct sinc table, 2 = cubic-interpolated table
__global__ __launch_bounds__(kTileOut) __attribute__((amdgpu_waves_per_eu(4))) void pv_resample_mfma_kernel(const ResArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    constexpr int NR = kResMfmaRows, NW = kTileOut / 64, NB = kResMfmaBlocks, NBW = kTileOut / 16 / NW;
    const float4 *tab4 = reinterpret_cast<const float4 *>(smem_raw);
    const float *stab = reinterpret_cast<const float *>(smem_raw);
    float *xs = reinterpret_cast<float *>(smem_raw + a.tab_bytes); // [nrl][xstride], then NW flag words
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const ResTile tile = a.tiles[blockIdx.x];
    const int row0 = blockIdx.y * NR, NF = a.filt_len, ncnt = tile.n_cnt, kcnt = tile.kcnt;
    const int nr = a.rows - row0 < NR ? a.rows - row0 : NR;
    const int nrl = a.rows < NR ? a.rows : NR; // rows the launch's LDS holds
    // (a tile too long for the padded layout stages at lds_floats and takes the vector loop.  No engine makes one, at
    // any pitch: a tile's 256 outputs span n_cnt <= floor(255 num/den) + 1 + filt_len samples, every engine sizes
    // lds_floats = (floor(256 num/den) + filt_len + 4 + 4 + 3) & ~3 >= n_cnt + 7, and the padded stride is
    // lds_floats - 2 (lds_floats is a multiple of 4), so n_cnt + 4 <= lds_floats - 3 < xstride.
    // tests/test_resample_rungs_host.py holds the inequality for -60 ... +60 semitones in 0.01 steps.)
    const bool fits = ncnt + 4 <= res_mfma_xstride(a.lds_floats);
    const int xstride = fits ? res_mfma_xstride(a.lds_floats) : a.lds_floats;
    const int nstage = fits ? ncnt + 4 : ncnt;
    const uint2 *__restrict__ ot = a.otab + (int64_t)blockIdx.x * kTileOut;
    const int q = lane >> 4, c = lane & 15;
    uint2 eo[NBW]; // the lane's output of each of its wave's blocks, loaded before the staging (blocks interleaved over
                   // the waves: a short tile stays balanced)
#pragma unroll
    for (int k = 0; k < NBW; ++k) {
        const int n = 16 * (w + NW * k) + c;
        eo[k] = n < kcnt ? ot[n] : make_uint2(0u, 0u);
    }
    bool bad = false;
    for (int i = tid; i < nstage; i += kTileOut) {
        const int64_t n = tile.n_lo + i; // the stream is zero before its first sample (skip_zeros, :1225)
        float xv[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const float *__restrict__ st = a.stream + (int64_t)(row0 + r) * ((int64_t)a.smask + 1);
            xv[r] = (r < nr && i < ncnt && n >= 0) ? st[(uint32_t)n & (uint32_t)a.smask] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < NR; ++r)
            if (r < nr) {
                xs[r * xstride + i] = xv[r];
                bad |= (__float_as_uint(xv[r]) & 0x7f800000u) == 0x7f800000u;
            }
    }
    if (kRes == 2) {
        const int cnt = a.oversample * (NF + 1);
        for (int i = tid; i < cnt; i += kTileOut) reinterpret_cast<float4 *>(smem_raw)[i] = a.tab4[i];
    } else {
        for (int i = tid; i < a.sinc_len; i += kTileOut) reinterpret_cast<float *>(smem_raw)[i] = a.sinc[i];
    }
    int *flag = reinterpret_cast<int *>(xs + nrl * xstride);
    const bool wave_bad = __any(bad);
    if (fits && lane == 0) flag[w] = wave_bad ? 1 : 0;
    __syncthreads();
    bool vec = !fits;
    if (fits) {
#pragma unroll
        for (int i = 0; i < NW; ++i) vec |= flag[i] != 0;
    }
    float *__restrict__ out = a.out + (int64_t)row0 * a.out_stride_row + (tile.k0 - a.k_base);
    if (vec) {
        if (tid < kcnt) res_fast_valu<kRes, NR>(a, ot[tid], xs, xstride, nr, tab4, stab, out + tid, nr);
        return;
    }
    const float *xa = xs + (c < nr ? c : 0) * xstride + q; // A: X[row c][t + q] (a missing row reads row 0)
#pragma unroll 1
    for (int p = 0; p < NBW / NB; ++p) {
        int base[NB], jb[NB], nk[NB], nb[NB];
        float4 cw[NB];
        const float4 *T[NB];
        const float *S[NB];
        int ks = 0;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const int n0 = 16 * (w + NW * (p * NB + b));
            const int n = n0 + c;
            const uint2 e = eo[p * NB + b];
            const int off = (int)(e.x & 0xffffu);
            const int last = (kcnt - 1 - n0 < 15 ? kcnt - 1 - n0 : 15); // uniform; < 0: an empty block
            base[b] = __builtin_amdgcn_readfirstlane(off);
            nk[b] = last < 0 ? 0 : (__builtin_amdgcn_readlane(off, last < 0 ? 0 : last) - base[b] + NF + 3) >> 2;
            ks = nk[b] > ks ? nk[b] : ks;
            // tap index of the lane's (t, n) at K-step s: j = jb + 4 s; outputs past kcnt never enter the band
            jb[b] = n < kcnt ? q - (off - base[b]) : -(1 << 29);
            nb[b] = n0;
            if constexpr (kRes == 2) {
                cw[b] = res_cubic_coef(__uint_as_float(e.y));
                T[b] = tab4 + (int)(e.x >> 16) * (NF + 1);
            } else {
                S[b] = stab + (e.x >> 16) * (uint32_t)NF;
            }
        }
        ks = __builtin_amdgcn_readfirstlane(ks);
        if (ks == 0) break; // (these blocks and every later one are past kcnt)
        v4f acc[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[b] = v4f{0.f, 0.f, 0.f, 0.f};
        auto step = [&](const int s) {
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                // (every lane reads a tap -- out of band a clamped one, then zeroed: no branch in the loop; a step past
                // the block's own span has zero taps, and its sample positions stop at the zero padding)
                const uint32_t j = (uint32_t)(jb[b] + 4 * s), jc = j < (uint32_t)(NF - 1) ? j : (uint32_t)(NF - 1);
                float h;
                if constexpr (kRes == 2) h = res_cubic_tap(cw[b], T[b][jc]);
                else h = S[b][jc];
                h = j < (uint32_t)NF ? h : 0.f;
                const int t = base[b] + 4 * s < ncnt ? base[b] + 4 * s : ncnt;
                acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[t], h, acc[b], 0, 0, 0);
            }
        };
        int s = 0; // (four steps per trip: the compiler does not unroll a loop of run-time length here)
#if defined(PV_EXP_RES) && (PV_EXP_RES & 4)
        s = ks; // (elimination build, timing only: bit 2 no K-steps -- staging, table copy, set-up and stores remain)
#endif
#pragma unroll 1
        for (; s + 4 <= ks; s += 4) step(s), step(s + 1), step(s + 2), step(s + 3);
#pragma unroll 1
        for (; s < ks; ++s) step(s);
        // D: lane l holds Out[row 4 (l>>4) + i][n0 + (l&15)] in element i
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const int n = nb[b] + c;
            if (n < kcnt) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (4 * q + i < nr) out[(int64_t)(4 * q + i) * a.out_stride_row + n] = acc[b][i];
            }
        }
    }
}

// (Measured and left out, round 3: NO = 4 consecutive outputs per thread walking the samples of their common span once
// -- the filter rows padded with zeros so that taps outside 0 .. NF - 1 contribute nothing -- four times fewer sample
// reads, bit-identical output.  Alone it is faster, 0.255 -> 0.202 ms per launch, its four 16-byte coefficient reads per
// sample step then being the LDS cost; beside the rotation chain, where the kernel really runs, its 64 KB of LDS per
// workgroup and low occupancy make it slower, 0.30 -> 0.34-0.38 ms: profiles/r03/resample_elim.txt.)
template <int NR> static void launch_resample_fast_rows(const ResArgs &a, size_t lds, hipStream_t st) {
    const dim3 grid(a.ntiles, (a.rows + NR - 1) / NR);
    if (a.interp) {
        launch_big_lds<pv_resample_fast_kernel<2, NR>>(grid, dim3(kTileOut), lds, st, a);
    } else {
        launch_big_lds<pv_resample_fast_kernel<1, NR>>(grid, dim3(kTileOut), lds, st, a);
    }
}
// The ladder, stated once: launch_resample launches what this returns, Core::init refuses what does not fit, and
// pv_debug_resample_rung reports it (pv_kernels.h).
ResRung resample_rung(const ResArgs &a) {
    const size_t fl = sizeof(float);
    const auto rows_lds = [&](int nr) { return (size_t)a.tab_bytes + fl * (size_t)a.lds_floats * nr; };
    const auto answer = [](int rung, size_t lds) { return ResRung{rung, lds, lds <= kMaxDynLds}; };
    if (!a.fast) return answer(kResRungRef4, rows_lds(kResRows));
    static const int rows_env = [] { // AUDIOMOD_PV_RES_ROWS=8|16 (tuning knob)
        const char *e = getenv("AUDIOMOD_PV_RES_ROWS");
        return e ? atoi(e) : 0;
    }();
    static const bool mfma = [] { // AUDIOMOD_PV_RES_MFMA=0: the vector kernel (for comparison; same bits)
        const char *e = getenv("AUDIOMOD_PV_RES_MFMA");
        return !(e && atoi(e) == 0);
    }();
    if (mfma && rows_lds(kResMfmaRows) <= 64 * 1024) {
        // LDS: the tables, then the staged rows -- at the padded stride plus the flag words, or at lds_floats for a
        // tile that does not fit it -- never more than the vector kernel's 16 rows x lds_floats for two rows or more
        const size_t nrl = a.rows < kResMfmaRows ? a.rows : kResMfmaRows;
        const size_t padded = fl * (nrl * res_mfma_xstride(a.lds_floats) + kTileOut / 64);
        return answer(kResRungMfma, (size_t)a.tab_bytes + std::max(fl * nrl * (size_t)a.lds_floats, padded));
    }
    const int want = rows_env ? rows_env : kResFastRows; // (8 -> 16 rows per thread: 0.265 -> 0.255 ms per launch alone, cfg4 -7 st +3 %)
    if (want >= 16 && a.rows >= 16 && rows_lds(16) <= 64 * 1024) return answer(kResRungVec16, rows_lds(16));
    return answer(kResRungVec8, rows_lds(8));
}

void launch_resample(const ResArgs &a, hipStream_t st) {
    if (a.ntiles <= 0) return; // (a group of dropped slices completes no output)
    const ResRung r = resample_rung(a); // (engine creation has refused what does not fit)
    census_resample_rung(0, r.rung, a.interp != 0, r.lds_bytes);
    if (r.rung == kResRungMfma) {
        const dim3 grid(a.ntiles, (a.rows + kResMfmaRows - 1) / kResMfmaRows);
        if (a.interp) {
            launch_big_lds<pv_resample_mfma_kernel<2>>(grid, dim3(kTileOut), r.lds_bytes, st, a);
        } else {
            launch_big_lds<pv_resample_mfma_kernel<1>>(grid, dim3(kTileOut), r.lds_bytes, st, a);
        }
    } else if (r.rung == kResRungVec16) {
        launch_resample_fast_rows<16>(a, r.lds_bytes, st);
    } else if (r.rung == kResRungVec8) {
        launch_resample_fast_rows<8>(a, r.lds_bytes, st);
    } else {
        const dim3 grid(a.ntiles, (a.rows + kResRows - 1) / kResRows);
        if (a.interp) {
            launch_big_lds<pv_resample_kernel<2>>(grid, dim3(kTileOut), r.lds_bytes, st, a);
        } else {
            launch_big_lds<pv_resample_kernel<1>>(grid, dim3(kTileOut), r.lds_bytes, st, a);
        }
    }
}

// --------------------------------------------------------------------------------------------
// The drop-in streaming path in ONE launch (opt-in, AUDIOMOD_PV_STREAM_LAUNCHES=single).  A 480-frame call of a
// stereo stream triggers two or three slices per channel: far too little work to fill the chip, and with one
// launch per stage the host spends ~7 us on each of five launches.  One workgroup of eight waves runs the stages
// back to back instead -- the same device functions as the batch kernels, frames / steps spread over the waves,
// rows and tiles looped -- with a workgroup barrier (and a fence: the stages hand data over through global
// memory) between stages.  Measured on MI355X it LOSES (93 vs 70 us per call, 513 vs 242 us at 4800-frame
// calls): the separate launches are asynchronous and already overlap the kernels, while a single workgroup pays
// every stage's latency in sequence on one CU.  Kept as a tested alternative, off by default.
// --------------------------------------------------------------------------------------------
constexpr int kStreamThreads = 512;

__device__ __forceinline__ void stage_handoff() {
    __threadfence();                  // later stages read what other waves of this workgroup wrote to global memory
    __builtin_amdgcn_s_dcache_inv();  // ... some of it through the scalar cache (wave-uniform counts and modes)
    __syncthreads();
}

template <int NC> __global__ __launch_bounds__(kStreamThreads) void pv_stream_kernel(const StreamArgs s) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = kStreamThreads / 64;
    const int Tn = s.aa.Tn, rows = s.aa.rows, work = rows * Tn;
    cf *wlds = reinterpret_cast<cf *>(smem_raw) + wave * WF<NC>::LDS_CF;
    for (int i = wave; i < work; i += nw)
        analyze_wave_role<NC, (kStreamThreads / 64) * WF<NC>::LDS_CF * sizeof(cf)>(s.aa, i / Tn, i % Tn, wlds);
    stage_handoff();
    if (s.coremode == 1) {
        // (slice-major order is not needed: a step only reads peak lists, all written by now)
        for (int i = wave; i < work; i += nw)
            match_wave_role(s.ma, i / Tn, i % Tn, smem_raw + (size_t)wave * match_wave_lds(s.ma.hs, s.ma.PKP));
        stage_handoff();
        for (int row = 0; row < rows; ++row) {
            seq_role<1>(s.qa, row, smem_raw);
            stage_handoff();
        }
    } else if (s.coremode == 0) {
        for (int row = 0; row < rows; ++row)
            for (int i = threadIdx.x; i < s.pa.hs; i += kStreamThreads) prop_role(s.pa, row, i);
        stage_handoff();
    }
    if (s.cepstral) {
        for (int i = wave; i < work; i += nw) cepstral_wave_role<NC>(s.ca, i / Tn, i % Tn, wlds);
        stage_handoff();
    }
    for (int i = wave; i < work; i += nw) synth_wave_role<NC>(s.sa, i / Tn, i % Tn, wlds);
    stage_handoff();
    for (int tile = 0; tile < s.oa.ntiles; ++tile)
        for (int row = 0; row < rows; ++row) {
            ola_role<1>(s.oa, tile, row, smem_raw);
            __syncthreads();
        }
}

static size_t stream_lds_bytes(const StreamArgs &s) {
    const size_t per_wave = (s.aa.tb.nc == 1024 ? WF<1024>::LDS_CF : WF<2048>::LDS_CF) * sizeof(cf);
    size_t lds = (kStreamThreads / 64) * per_wave + 4 * PV_ATAN_BLOB_WORDS; // + atan2f's interval table
    const size_t m = (kStreamThreads / 64) * match_wave_lds(s.ma.hs, s.ma.PKP);
    if (s.coremode == 1 && m > lds) lds = m;
    if (s.coremode == 1 && seq_lds_bytes(s.qa) > lds) lds = seq_lds_bytes(s.qa);
    if (ola_lds_bytes(s.oa, 1) > lds) lds = ola_lds_bytes(s.oa, 1);
    return lds;
}

bool stream_kernel_supported(const StreamArgs &s) {
    return (s.aa.tb.nc == 1024 || s.aa.tb.nc == 2048) && stream_lds_bytes(s) <= kMaxDynLds;
}

// The wave-per-frame analysis code addresses atan2f's table by a compile-time LDS address, which is right only while
// the kernels that contain it have no static LDS (their dynamic LDS then starts at 0).  The engine asks once per
// device, at creation.
bool lds_starts_at_zero() {
    const void *ks[] = {reinterpret_cast<const void *>(pv_analyze_wave_kernel<256, 1>),
                        reinterpret_cast<const void *>(pv_analyze_wave_kernel<512, 1>),
                        reinterpret_cast<const void *>(pv_analyze_wave_kernel<1024, 1>),
                        reinterpret_cast<const void *>(pv_analyze_wave_kernel<2048, 1>),
                        reinterpret_cast<const void *>(pv_stream_kernel<1024>),
                        reinterpret_cast<const void *>(pv_stream_kernel<2048>)};
    for (const void *k : ks) {
        hipFuncAttributes fa{};
        if (hipFuncGetAttributes(&fa, k) != hipSuccess || fa.sharedSizeBytes != 0) return false;
    }
    return true;
}

void launch_stream(const StreamArgs &s, hipStream_t st) {
    const size_t lds = stream_lds_bytes(s);
    if (s.coremode == 1) census_phase(0, kPhaseFormStream, 1); // (seq_role<1> on the kernel's 512 threads)
    census_analysis_kernel(0, kAnaKernelStream, s.aa.tb.nc);
    if (s.cepstral) census_cepstral(0, kCepKernelWave, s.aa.tb.nc);
    if (s.aa.tb.nc == 1024) {
        launch_big_lds<pv_stream_kernel<1024>>(dim3(1), dim3(kStreamThreads), lds, st, s);
    } else {
        launch_big_lds<pv_stream_kernel<2048>>(dim3(1), dim3(kStreamThreads), lds, st, s);
    }
}

// --------------------------------------------------------------------------------------------
// Stream pool (pv_kernels.h PoolSlot): the streaming path's stages for many independent streams in one launch each.
// Every workgroup reads its slot's entry, builds a slot view of the argument block and calls the device functions the
// batch kernels call, so a slot computes exactly what a single-stream engine computes.  Slots differ in their slice
// counts: a workgroup past its slot's Tn (or tile count) returns at once (workgroup-uniform).
// --------------------------------------------------------------------------------------------
// The per-slot kernels' copies of the bodies of pv_synth_chain_kernel, pv_resample_kernel and pv_resample_fast_kernel,
// as device functions of the row / (tile, row group): the batch kernels keep their source, and so their machine code,
// exactly as they are.  A change to one of those kernels must be made to its copy here too.
template <int NC, int kPlainCore, int kRes, bool kFast>
__device__ __forceinline__ void pool_synth_chain_role(const SynthArgs &s, const ChainArgs &c, const int row, char *smem_raw,
                                                      const int run = 0, const bool last_run = true) {
    using W = WF<NC>;
    constexpr int N = 2 * NC, hs = NC, NQ = N / 4, NP = NQ / 64;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    // (the pools: a slot's slices of a launch are one run, run 0; the mixed batch splits them, pv_kernels.h MbSlot)
    // (entry i of the run's list is its i-th slice in order; ChainSlice::tl says which slice of the launch it is)
    const int i_begin = c.run_off[run], i_count = c.run_off[run + 1] - i_begin;
    cf *wlds = reinterpret_cast<cf *>(smem_raw) + wave * W::LDS_CF;
    const ChainLds l = chain_carve(c, smem_raw + (size_t)c.waves * W::LDS_CF * sizeof(cf));
    chain_prologue(c, l, row, run == 0);
    const float *__restrict__ w = s.tb.window;
    const bool upper = (row % c.C) > 0;
    const int lane0 = lane;
    for (int i = wave; i < i_count; i += c.waves) {
        // the lane id, made opaque once per iteration: everything derived from it is recomputed per slice instead of
        // being hoisted out of the loop and held in registers (which spilled ~100 VGPRs)
        int lane = lane0;
        asm volatile("" : "+v"(lane));
        const ChainSlice sl = c.slices[i_begin + i];
        const int tl = sl.tl;
        const bool skip = (sl.flags & 1) && upper; // wave-uniform
        float4 A[NP];
        if (!skip) {
            if (!PV_CHAIN_DIAG(c, 8)) synth_wave_role<NC, kPlainCore, 1, kFast>(s, row, tl, wlds, lane);
            // ifftshift + synthesis window (phasevocoderimpl.h:183-198): four consecutive samples per lane and piece
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                const int i = 4 * (lane + 64 * j);
                const int e = ((i + hs) & (N - 1)) >> 1;
                const cf z0 = wlds[W::pad(e)], z1 = wlds[W::pad(e) + 1];
                const float4 ww = *reinterpret_cast<const float4 *>(w + i);
                A[j] = make_float4(z0.x * ww.x, z0.y * ww.y, z1.x * ww.z, z1.y * ww.w);
            }
        }
        const int r = sl.acc_pos & 3; // wave-uniform
        if (r == 0) chain_slice_tail<0, NP, kRes, kFast>(c, l, sl, A, skip, row, i, lane);
        else if (r == 1) chain_slice_tail<1, NP, kRes, kFast>(c, l, sl, A, skip, row, i, lane);
        else if (r == 2) chain_slice_tail<2, NP, kRes, kFast>(c, l, sl, A, skip, row, i, lane);
        else chain_slice_tail<3, NP, kRes, kFast>(c, l, sl, A, skip, row, i, lane);
    }
    chain_epilogue(c, l, row, last_run);
}

template <int kRes> // 1 = direct sinc table, 2 = cubic-interpolated table
__device__ __forceinline__ void pool_resample_role(const ResArgs &a, const unsigned tile_i, const unsigned grp, char *smem_raw) {
    constexpr int NR = kResRows;
    float4 *tab4 = reinterpret_cast<float4 *>(smem_raw);
    float *stab = reinterpret_cast<float *>(smem_raw);
    float *xs = reinterpret_cast<float *>(smem_raw + a.tab_bytes); // [NR][lds_floats]
    const int nt = blockDim.x, tid = threadIdx.x;
    const ResTile tile = a.tiles[tile_i];
    const int row0 = grp * NR, NF = a.filt_len;
    const int nr = a.rows - row0 < NR ? a.rows - row0 : NR;
    uint2 oe = make_uint2(0u, 0u);
    if (tid < tile.kcnt) oe = a.otab[(int64_t)tile_i * kTileOut + tid];
    // the tile's stream samples of every row, all loads in flight before the first LDS write (a tile needs at most
    // two samples per thread and row at the ratios that resample: n_cnt <= 256 * num/den + filt_len)
    float xv[NR][2];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const float *__restrict__ st = a.stream + (int64_t)(r < nr ? row0 + r : row0) * ((int64_t)a.smask + 1);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int i = tid + h * kTileOut;
            const int64_t n = tile.n_lo + i; // the stream is zero before its first sample (skip_zeros, :1225)
            xv[r][h] = (i < tile.n_cnt && n >= 0) ? st[(uint32_t)n & (uint32_t)a.smask] : 0.f;
        }
    }
    if (kRes == 2) {
        const int cnt = a.oversample * (NF + 1);
        for (int i = tid; i < cnt; i += nt) tab4[i] = a.tab4[i];
    } else {
        for (int i = tid; i < a.sinc_len; i += nt) stab[i] = a.sinc[i];
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int i = tid + h * kTileOut;
            if (i < tile.n_cnt) xs[r * a.lds_floats + i] = xv[r][h];
        }
    }
    // (longer tiles -- strong down-sampling, more than two samples per thread -- take the rest in a loop)
    for (int i = tid + 2 * kTileOut; i < tile.n_cnt; i += nt)
        for (int r = 0; r < nr; ++r) {
            const int64_t n = tile.n_lo + i;
            const float *__restrict__ st = a.stream + (int64_t)(row0 + r) * ((int64_t)a.smask + 1);
            xs[r * a.lds_floats + i] = n >= 0 ? st[(uint32_t)n & (uint32_t)a.smask] : 0.f;
        }
    __syncthreads();
    if (tid >= tile.kcnt) return;
    float *__restrict__ out = a.out + (int64_t)row0 * a.out_stride_row + (tile.k0 - a.k_base) + tid;
    const float *x = xs + (int)(oe.x & 0xffffu); // tap j = 0
    if (kRes == 2) {
        const float frac = __uint_as_float(oe.y);
        const float4 *__restrict__ T = tab4 + (int)(oe.x >> 16) * (NF + 1);
        v2f a01[NR], a23[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) a01[r] = v2f{0.f, 0.f}, a23[r] = v2f{0.f, 0.f};
#pragma unroll 4
        for (int j = 0; j < NF; ++j) { // NF is a multiple of 4 (resample.c:687)
            const float4 c = T[j];
            const v2f c01 = {c.x, c.y}, c23 = {c.z, c.w};
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const float xr = x[r * a.lds_floats + j]; // a missing row holds zeros: computed, never stored
                const v2f xx = {xr, xr};
                a01[r] += xx * c01;
                a23[r] += xx * c23;
            }
        }
        // cubic_coef (resample.c:339-351)
        const float c0 = -0.16667f * frac + 0.16667f * frac * frac * frac;
        const float c1 = frac + 0.5f * frac * frac - 0.5f * frac * frac * frac;
        const float c3 = -0.33333f * frac + 0.5f * frac * frac - 0.16667f * frac * frac * frac;
        const float c2 = (float)(1. - c0 - c1 - c3);
#pragma unroll
        for (int r = 0; r < NR; ++r)
            if (r < nr)
                out[(int64_t)r * a.out_stride_row] = (c0 * a01[r].x) + (c1 * a01[r].y) + (c2 * a23[r].x) + (c3 * a23[r].y);
    } else {
        const float *t = stab + (oe.x >> 16) * (uint32_t)NF;
        for (int r = 0; r < nr; ++r) {
            float sum = 0.f;
            for (int j = 0; j < NF; ++j) sum += x[r * a.lds_floats + j] * t[j];
            out[(int64_t)r * a.out_stride_row] = sum;
        }
    }
}

template <int kRes, int NR> // 1 = direct sinc table, 2 = cubic-interpolated table
__device__ __forceinline__ void pool_resample_fast_role(const ResArgs &a, const unsigned tile_i, const unsigned grp, char *smem_raw) {
    float4 *tab4 = reinterpret_cast<float4 *>(smem_raw);
    float *stab = reinterpret_cast<float *>(smem_raw);
    float *xs = reinterpret_cast<float *>(smem_raw + a.tab_bytes); // [NR][lds_floats]
    const int nt = blockDim.x, tid = threadIdx.x;
    const ResTile tile = a.tiles[tile_i];
    const int row0 = grp * NR, NF = a.filt_len;
    const int nr = a.rows - row0 < NR ? a.rows - row0 : NR;
    uint2 oe = make_uint2(0u, 0u);
    if (tid < tile.kcnt) oe = a.otab[(int64_t)tile_i * kTileOut + tid];
    // the tile's stream samples of every row (a missing row re-reads the group's first: computed, never stored)
    for (int i = tid; i < tile.n_cnt; i += nt) {
        const int64_t n = tile.n_lo + i; // the stream is zero before its first sample (skip_zeros, :1225)
        float xv[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const float *__restrict__ st = a.stream + (int64_t)(r < nr ? row0 + r : row0) * ((int64_t)a.smask + 1);
            xv[r] = n >= 0 ? st[(uint32_t)n & (uint32_t)a.smask] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) xs[r * a.lds_floats + i] = xv[r];
    }
    if (kRes == 2) {
        const int cnt = a.oversample * (NF + 1);
        for (int i = tid; i < cnt; i += nt) tab4[i] = a.tab4[i];
    } else {
        for (int i = tid; i < a.sinc_len; i += nt) stab[i] = a.sinc[i];
    }
    __syncthreads();
    if (tid >= tile.kcnt) return;
    float *__restrict__ out = a.out + (int64_t)row0 * a.out_stride_row + (tile.k0 - a.k_base) + tid;
    const float *x = xs + (int)(oe.x & 0xffffu); // tap j = 0
    float acc[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = 0.f;
    if (kRes == 2) {
        const float frac = __uint_as_float(oe.y);
        // cubic_coef (resample.c:339-351)
        const float c0 = -0.16667f * frac + 0.16667f * frac * frac * frac;
        const float c1 = frac + 0.5f * frac * frac - 0.5f * frac * frac * frac;
        const float c3 = -0.33333f * frac + 0.5f * frac * frac - 0.16667f * frac * frac * frac;
        const float c2 = (float)(1. - c0 - c1 - c3);
        const float4 *__restrict__ T = tab4 + (int)(oe.x >> 16) * (NF + 1);
#pragma unroll 4
        for (int j = 0; j < NF; ++j) { // NF is a multiple of 4 (resample.c:687)
            // (PV_EXP_RES: elimination builds for timing only -- bit 0 no sample reads, bit 1 no coefficient reads)
#if defined(PV_EXP_RES) && (PV_EXP_RES & 2)
            const float4 c = make_float4(frac, c0, c1, (float)j);
#else
            const float4 c = T[j];
#endif
            const float h = __builtin_fmaf(c3, c.w, __builtin_fmaf(c2, c.z, __builtin_fmaf(c1, c.y, c0 * c.x)));
#pragma unroll
            for (int r = 0; r < NR; ++r) {
#if defined(PV_EXP_RES) && (PV_EXP_RES & 1)
                acc[r] = __builtin_fmaf(frac + (float)r, h, acc[r]);
#else
                acc[r] = __builtin_fmaf(x[r * a.lds_floats + j], h, acc[r]);
#endif
            }
        }
    } else {
        const float *t = stab + (oe.x >> 16) * (uint32_t)NF;
#pragma unroll 4
        for (int j = 0; j < NF; ++j) {
            const float h = t[j];
#pragma unroll
            for (int r = 0; r < NR; ++r) acc[r] = __builtin_fmaf(x[r * a.lds_floats + j], h, acc[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < NR; ++r)
        if (r < nr) out[(int64_t)r * a.out_stride_row] = acc[r];
}

// input ingest (PoolIngest): one lane per sample, grid (ceil(max n / 256), C, entries); the source is the pool's packed
// staging buffer or, for pv_pool_feed_device, the caller's pitched device buffer of either wire type (converted on load)
__device__ __forceinline__ float pool_wire_load(float v) { return v; }
__device__ __forceinline__ float pool_wire_load(int16_t v) { return pv_wire_i16_to_f32(v); }
template <typename T>
__device__ __forceinline__ void pool_ingest(const T *__restrict__ src, float *__restrict__ ring, const int ring_len,
                                            const PoolIngest *__restrict__ ents) {
    const PoolIngest e = ents[blockIdx.z];
    const int i = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    if (i >= e.n) return;
    ring[(int64_t)(e.row0 + c) * ring_len + ((e.pos + i) & (int64_t)(ring_len - 1))] =
        pool_wire_load(src[e.src_off + c * e.src_pitch + i]);
}
__global__ __launch_bounds__(256) void pv_pool_ingest_kernel(const float *__restrict__ src, float *__restrict__ ring,
                                                             const int ring_len, const PoolIngest *__restrict__ ents) {
    pool_ingest(src, ring, ring_len, ents);
}
__global__ __launch_bounds__(256) void pv_pool_ingest_i16_kernel(const int16_t *__restrict__ src, float *__restrict__ ring,
                                                                 const int ring_len, const PoolIngest *__restrict__ ents) {
    pool_ingest(src, ring, ring_len, ents);
}

void launch_pool_ingest(const void *src, int wire, float *ring, int ring_len, int C, const PoolIngest *ents, int nents,
                        int max_n, hipStream_t st) {
    if (nents <= 0 || max_n <= 0) return;
    const dim3 grid((max_n + 255) / 256, C, nents);
    if (wire == PV_WIRE_I16)
        hipLaunchKernelGGL(pv_pool_ingest_i16_kernel, grid, dim3(256), 0, st, static_cast<const int16_t *>(src), ring,
                           ring_len, ents);
    else
        hipLaunchKernelGGL(pv_pool_ingest_kernel, grid, dim3(256), 0, st, static_cast<const float *>(src), ring, ring_len,
                           ents);
}

// int16 egress (PoolEgress): one lane per sample, neighbouring lanes write neighbouring int16 (a wave covers 128
// contiguous bytes of a row; rows of an arbitrary pitch start on 2-byte boundaries only, so nothing wider is assumed)
__global__ __launch_bounds__(256) void pv_pool_egress_i16_kernel(const float *__restrict__ arena, int16_t *__restrict__ dst,
                                                                 const PoolEgress *__restrict__ ents) {
    const PoolEgress e = ents[blockIdx.z];
    const int i = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    if (i >= e.n) return;
    dst[e.dst_off + c * e.dst_pitch + i] = pv_wire_f32_to_i16(arena[e.src_off + c * e.src_pitch + i]);
}

void launch_pool_egress_i16(const float *arena, int16_t *dst, int C, const PoolEgress *ents, int nents, int max_n,
                            hipStream_t st) {
    if (nents <= 0 || max_n <= 0) return;
    hipLaunchKernelGGL(pv_pool_egress_i16_kernel, dim3((max_n + 255) / 256, C, nents), dim3(256), 0, st, arena, dst, ents);
}

// snapshot gather / scatter (SnapSeg): pure streaming, no arithmetic and no LDS; workgroup (x, y) is part y of segment x
__global__ __launch_bounds__(256) void pv_pool_snapshot_kernel(const SnapArgs a) {
    const SnapSeg s = a.segs[blockIdx.x];
    char *const b = a.bufs[s.buf] + s.buf_off, *const g = a.stage + s.stage_off;
    const char *__restrict__ src = a.to_stage ? b : g;
    char *__restrict__ dst = a.to_stage ? g : b;
    const int64_t tid = (int64_t)blockIdx.y * 256 + threadIdx.x, nt = (int64_t)gridDim.y * 256;
    if ((((uintptr_t)src | (uintptr_t)dst | (uintptr_t)s.bytes) & 15) == 0) {
        const float4 *__restrict__ s4 = reinterpret_cast<const float4 *>(src);
        float4 *__restrict__ d4 = reinterpret_cast<float4 *>(dst);
        for (int64_t i = tid; i < (s.bytes >> 4); i += nt) d4[i] = s4[i];
    } else {
        const uint32_t *__restrict__ s1 = reinterpret_cast<const uint32_t *>(src);
        uint32_t *__restrict__ d1 = reinterpret_cast<uint32_t *>(dst);
        for (int64_t i = tid; i < (s.bytes >> 2); i += nt) d1[i] = s1[i];
    }
}

void launch_pool_snapshot(const SnapArgs &a, int nsegs, int parts, hipStream_t st) {
    if (nsegs <= 0) return;
    hipLaunchKernelGGL(pv_pool_snapshot_kernel, dim3(nsegs, parts < 1 ? 1 : parts), dim3(256), 0, st, a);
}

__device__ __forceinline__ AnalyzeArgs pool_view(const AnalyzeArgs &a, const PoolSlot &ps) {
    AnalyzeArgs v = a;
    const int64_t r = ps.row0;
    v.t0 = ps.t0, v.s0 = ps.s0, v.Tn = ps.Tn;
    v.ia.in += r * a.ia.stride_c;
    v.mag += r * a.TR * a.tb.HP;
    v.phase += r * a.TR * a.tb.HP;
    if (a.find_peaks) {
        v.peaks += r * a.TR * a.PKP;
        v.npk += r * a.TR;
    }
    return v;
}

// analysis, one wave per frame: workgroup x = tl * C + c
template <int NC> __global__ __launch_bounds__(64) void pv_pool_analyze_wave_kernel(const AnalyzeArgs a, const PoolLaunch p) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    const PoolSlot ps = p.slots[blockIdx.y];
    const int tl = __builtin_amdgcn_readfirstlane((int)blockIdx.x / a.rows), row = blockIdx.x - tl * a.rows;
    if (tl >= ps.Tn) return;
    analyze_wave_role<NC, WF<NC>::LDS_CF * sizeof(cf)>(pool_view(a, ps), row, tl, reinterpret_cast<cf *>(smem_raw));
}
__global__ __launch_bounds__(128) void pv_pool_analyze_split_kernel(const AnalyzeArgs a, const PoolLaunch p) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    const PoolSlot ps = p.slots[blockIdx.y];
    const int tl = __builtin_amdgcn_readfirstlane((int)blockIdx.x / a.rows), row = blockIdx.x - tl * a.rows;
    if (tl >= ps.Tn) return;
    analyze_split_role<WF2048S, WF2048S::LDS_CF * sizeof(cf)>(pool_view(a, ps), row, tl, reinterpret_cast<cf *>(smem_raw));
}

// The slot-table analysis launch of all three sets (pool, pmix, mb): grid (rows * frames, slots), one wave per frame
// or, at 4096 points with a.split, two.  `Set` names the set's two kernels (set.wave<NC, kBigLds>, set.split) and
// appends its trailing arguments.  Only the 4096-point wave kernel needs more than the default dynamic LDS.
template <class Set> static bool launch_slot_analyze(const Set &set, const AnalyzeArgs &a, const PoolLaunch &p, hipStream_t st) {
    const dim3 grid(a.rows * p.max_tn, p.nslots);
    const size_t atab = 4 * PV_ATAN_BLOB_WORDS;
    if (census_nc_index(a.tb.nc) >= 0) {
        census_analyze(Set::census_set, a.tb.nc, a.tb.nc == 2048 && a.split);
        census_analysis_kernel(Set::census_set, a.tb.nc == 2048 && a.split ? kAnaKernelSplit : kAnaKernelWave, a.tb.nc);
    }
    switch (a.tb.nc) {
    case 256: set.template wave<256, false>(grid, WF<256>::LDS_CF * sizeof(cf) + atab, st, a); return true;
    case 512: set.template wave<512, false>(grid, WF<512>::LDS_CF * sizeof(cf) + atab, st, a); return true;
    case 1024: set.template wave<1024, false>(grid, WF<1024>::LDS_CF * sizeof(cf) + atab, st, a); return true;
    case 2048:
        if (a.split) set.split(grid, WF2048S::LDS_CF * sizeof(cf) + atab + 64, st, a);
        else set.template wave<2048, true>(grid, WF<2048>::LDS_CF * sizeof(cf) + atab, st, a);
        return true;
    default: return false;
    }
}
struct PoolAnalyzeSet { // trailing argument p
    static constexpr int census_set = 1;
    const PoolLaunch &p;
    template <int NC, bool kBigLds> void wave(dim3 grid, size_t lds, hipStream_t st, const AnalyzeArgs &a) const {
        launch_maybe_big_lds<pv_pool_analyze_wave_kernel<NC>, kBigLds>(grid, dim3(64), lds, st, a, p);
    }
    void split(dim3 grid, size_t lds, hipStream_t st, const AnalyzeArgs &a) const {
        hipLaunchKernelGGL(pv_pool_analyze_split_kernel, grid, dim3(WF2048S::LANES), lds, st, a, p);
    }
};
bool launch_pool_analyze(const AnalyzeArgs &a, const PoolLaunch &p, hipStream_t st) {
    return launch_slot_analyze(PoolAnalyzeSet{p}, a, p, st);
}

// Cepstral formant shift of the slots' magnitude planes (the formant setting of the pools and the mixed batch,
// pv_*_set_formant): one wave per (row, slice) of a slot, workgroup x = tl * C + c as in the analysis kernel above.  The
// stage reads the slot table and the planes and nothing else of a set, so the three sets share this kernel.  A slot
// whose env_comp is 0 does not run the stage: its workgroups read the entry and return.
template <int NC>
__global__ __launch_bounds__(64) void pv_slot_cepstral_wave_kernel(const CepstralArgs a, const PoolLaunch p) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    const PoolSlot ps = p.slots[blockIdx.y];
    const int tl = __builtin_amdgcn_readfirstlane((int)blockIdx.x / a.rows), row = blockIdx.x - tl * a.rows;
    if (tl >= ps.Tn || ps.env_comp == 0.f) return; // wave-uniform
    CepstralArgs v = a;
    v.mag += (int64_t)ps.row0 * a.TR * a.tb.HP;
    v.Tn = ps.Tn, v.s0 = ps.s0, v.env_comp = ps.env_comp;
    cepstral_wave_role<NC>(v, row, tl, reinterpret_cast<cf *>(smem_raw));
}
bool launch_slot_cepstral(const CepstralArgs &a, const PoolLaunch &p, int census_set, hipStream_t st) {
    const dim3 grid(a.rows * p.max_tn, p.nslots);
    if (census_nc_index(a.tb.nc) < 0 || p.nslots <= 0 || p.max_tn <= 0) return false;
    census_cepstral(census_set, kCepKernelSlot, a.tb.nc);
    switch (a.tb.nc) {
    case 256: hipLaunchKernelGGL((pv_slot_cepstral_wave_kernel<256>), grid, dim3(64), WF<256>::LDS_CF * sizeof(cf), st, a, p); break;
    case 512: hipLaunchKernelGGL((pv_slot_cepstral_wave_kernel<512>), grid, dim3(64), WF<512>::LDS_CF * sizeof(cf), st, a, p); break;
    case 1024: hipLaunchKernelGGL((pv_slot_cepstral_wave_kernel<1024>), grid, dim3(64), WF<1024>::LDS_CF * sizeof(cf), st, a, p); break;
    default: hipLaunchKernelGGL((pv_slot_cepstral_wave_kernel<2048>), grid, dim3(64), WF<2048>::LDS_CF * sizeof(cf), st, a, p); break;
    }
    return true;
}

// phase-locked mode: match + rotation chain of a slot's rows (pv_phase_kernel), one workgroup per (channel, slot)
constexpr int kPoolSeqDepth = 8;
template <int D> __global__ __launch_bounds__(1024) void pv_pool_phase_kernel(const MatchArgs m, const SeqArgs a, const PoolLaunch p) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    const PoolSlot ps = p.slots[blockIdx.y];
    const int64_t r = ps.row0;
    const int32_t *pinc = reinterpret_cast<const int32_t *>(p.desc + ps.pinc_off);
    MatchArgs mv = m;
    mv.t0 = ps.t0, mv.s0 = ps.s0, mv.Tn = ps.Tn, mv.phase_inc = pinc;
    mv.phase += r * m.TR * m.HP;
    mv.peaks += r * m.TR * m.PKP;
    mv.npk += r * m.TR;
    mv.recs += r * m.TR * m.PKP;
    mv.modes += r * m.TR;
    SeqArgs av = a;
    av.t0 = ps.t0, av.s0 = ps.s0, av.Tn = ps.Tn, av.phase_inc = pinc;
    av.phase = mv.phase, av.peaks = mv.peaks, av.npk = mv.npk, av.recs = mv.recs, av.modes = mv.modes;
    av.rot += r * a.TR * a.PKP;
    av.outphase += r * a.TR * a.HP;
    av.st_kind += r;
    av.st_rot += r * a.PKP;
    av.st_po += r * a.hs;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
    for (int tl = wave; tl < mv.Tn; tl += nw)
        match_wave_role(mv, blockIdx.x, tl, smem_raw + (size_t)wave * match_wave_lds(mv.hs, mv.PKP));
    __threadfence(); // the records go through global memory: the chain's loads must see them
    __syncthreads();
    if (av.high_prio) __builtin_amdgcn_s_setprio(3);
    seq_role_ring<D>(av, blockIdx.x, smem_raw);
}

static size_t pool_phase_lds(int hs, int PKP) {
    SeqArgs q{};
    q.hs = hs, q.PKP = PKP;
    const int nt = seq_threads(PKP);
    const size_t seq_l = ((seq_lds_bytes(q) + 15) & ~(size_t)15) + (size_t)kPoolSeqDepth * nt * sizeof(PeakRec);
    const size_t match_l = (size_t)(nt / 64) * match_wave_lds(hs, PKP);
    return seq_l > match_l ? seq_l : match_l;
}
bool pool_phase_supported(int hs, int PKP) { return PKP <= seq_threads(PKP) && pool_phase_lds(hs, PKP) <= kMaxDynLds; }

bool launch_pool_phase(const MatchArgs &m, const SeqArgs &a, const PoolLaunch &p, hipStream_t st) {
    if (!pool_phase_supported(a.hs, a.PKP)) return false;
    census_phase(1, kPhaseFormFused, kPoolSeqDepth);
    launch_big_lds<pv_pool_phase_kernel<kPoolSeqDepth>>(dim3(a.rows, p.nslots), dim3(seq_threads(a.PKP)),
                       pool_phase_lds(a.hs, a.PKP), st, m, a, p);
    return true;
}

// coremode 0: the per-bin recurrence; grid (bins / 256, C, slots)
__global__ __launch_bounds__(kPropThreads) void pv_pool_prop_kernel(const PropArgs a, const PoolLaunch p) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const PoolSlot ps = p.slots[blockIdx.z];
    const int64_t r = ps.row0;
    PropArgs v = a;
    v.t0 = ps.t0, v.s0 = ps.s0, v.Tn = ps.Tn;
    v.phase_inc = reinterpret_cast<const int32_t *>(p.desc + ps.pinc_off);
    v.phase += r * a.TR * a.HP;
    v.outphase += r * a.TR * a.HP;
    v.st_pp += r * a.hs;
    v.st_po += r * a.hs;
    if (i < a.hs) prop_role(v, blockIdx.y, i);
}

bool launch_pool_prop(const PropArgs &a, const PoolLaunch &p, hipStream_t st) {
    hipLaunchKernelGGL(pv_pool_prop_kernel, dim3((a.hs + kPropThreads - 1) / kPropThreads, a.rows, p.nslots),
                       dim3(kPropThreads), 0, st, a, p);
    return true;
}

// fused synthesis + overlap-add: one workgroup per (channel, slot), one run (the slot's few slices)
// At most twelve waves per workgroup (the batch kernel's sixteen at fft 512 ... 2048): the slot view costs registers,
// and with 128 VGPRs per lane the fft 2048 variants spilled.  A slot's launch has at most kStreamChunk slices, and the
// number of waves does not change what the kernel computes (frames are added in slice order whatever the wave count).
constexpr int pool_chain_max_threads(int NC, int kPlainCore, bool kFast) {
    return chain_kernel_max_threads(NC, kPlainCore, kFast) < 768 ? chain_kernel_max_threads(NC, kPlainCore, kFast) : 768;
}
template <int NC, int kPlainCore, int kRes, bool kFast>
__global__ __launch_bounds__(pool_chain_max_threads(NC, kPlainCore, kFast)) void pv_pool_synth_chain_kernel(
    const SynthArgs s, const ChainArgs c, const PoolLaunch p) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    const PoolSlot ps = p.slots[blockIdx.y];
    const int64_t r = ps.row0;
    SynthArgs sv = s;
    sv.t0 = ps.t0, sv.s0 = ps.s0, sv.Tn = ps.Tn;
    sv.phase_inc = reinterpret_cast<const int32_t *>(p.desc + ps.pinc_off);
    const int64_t plane = r * s.TR * s.tb.HP;
    sv.mag += plane;
    sv.phase += plane;
    if (sv.outphase) sv.outphase += plane;
    if (sv.peaks) sv.peaks += r * s.TR * s.PKP;
    if (sv.npk) sv.npk += r * s.TR;
    if (sv.modes) sv.modes += r * s.TR;
    if (sv.rot) sv.rot += r * s.TR * s.PKP;
    if constexpr (kPlainCore < 0) { // the voice setting: a whisper slot of a ROBOTIC object reads its drawn phases
        sv.whisper = (s.whisper && ps.wh_off >= 0) ? s.whisper + ps.wh_off : nullptr;
        if (sv.whisper) sv.robotic = 0;
        // the carrier setting: a carrier slot is a channel vocoder over its own carrier planes (band length as derive())
        if (s.cmag && ps.car_off >= 0) {
            sv.cmag = s.cmag + ps.car_off, sv.cphase = s.cphase + ps.car_off;
            sv.voc_band_len = (2 * NC) / 1024;
            sv.robotic = 0;
        }
    }
    ChainArgs cv = c;
    cv.Tn = ps.Tn;
    cv.t0 = ps.t0;
    cv.slices = reinterpret_cast<const ChainSlice *>(p.desc + ps.cs_off);
    cv.run_off = reinterpret_cast<const int32_t *>(p.desc + ps.ro_off);
    cv.wden = reinterpret_cast<const float *>(p.desc + ps.wden_off);
    cv.wden_hi = cv.wden;
    cv.st_acc += 2 * r * c.AR; // [slot][2][C][AR]
    cv.acc_sel = ps.acc_sel;
    if (kRes) cv.stream += r * ((int64_t)c.smask + 1);
    cv.out = p.out + ps.out_off;
    cv.out_stride_row = ps.out_stride_row;
    pool_synth_chain_role<NC, kPlainCore, kRes, kFast>(sv, cv, blockIdx.x, smem_raw);
}

// The slot-table sets clamp the launch to the kernel's bounds (no launch below one wave).
static bool slot_chain_fit_waves(ChainArgs &c, int max_threads) {
    if (64 * c.waves > max_threads) c.waves = max_threads / 64;
    return c.waves >= 1;
}
struct PoolChainSet { // grid (rows, slots); trailing argument p
    static constexpr int census_set = 1;
    const SynthArgs &s;
    const PoolLaunch &p;
    hipStream_t st;
    static constexpr int max_threads(int NC, int kPlainCore, bool kFast) { return pool_chain_max_threads(NC, kPlainCore, kFast); }
    static bool fit_waves(ChainArgs &c, int max_threads) { return slot_chain_fit_waves(c, max_threads); }
    template <int NC, int kPlainCore, int kRes, bool kFast> void launch(const ChainArgs &c, dim3 block, size_t lds) const {
        launch_big_lds<pv_pool_synth_chain_kernel<NC, kPlainCore, kRes, kFast>>(dim3(c.rows, p.nslots), block, lds, st, s, c, p);
    }
};
bool launch_pool_synth_chain(const SynthArgs &s, const ChainArgs &c, const PoolLaunch &p, hipStream_t st, bool launch) {
    return launch_chain(PoolChainSet{s, p, st}, s, s.tb.nc, c, launch);
}

// resampling: grid (tiles, row groups, slots)
__device__ __forceinline__ bool pool_res_view(const ResArgs &a, const PoolLaunch &p, ResArgs &v) {
    const PoolSlot ps = p.slots[blockIdx.z];
    if ((int)blockIdx.x >= ps.res_ntiles) return false;
    v = a;
    v.ntiles = ps.res_ntiles;
    v.stream += (int64_t)ps.row0 * ((int64_t)a.smask + 1);
    v.tiles = reinterpret_cast<const ResTile *>(p.desc + ps.res_off);
    v.otab = reinterpret_cast<const uint2 *>(p.desc + ps.otab_off);
    v.out = p.out + ps.out_off;
    v.out_stride_row = ps.out_stride_row;
    v.k_base = ps.k_base;
    return true;
}
template <int kRes> __global__ __launch_bounds__(kTileOut) void pv_pool_resample_kernel(const ResArgs a, const PoolLaunch p) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    ResArgs v;
    if (!pool_res_view(a, p, v)) return;
    pool_resample_role<kRes>(v, blockIdx.x, blockIdx.y, smem_raw);
}
constexpr int kPoolResFastRows = 8;
template <int kRes> __global__ __launch_bounds__(kTileOut) void pv_pool_resample_fast_kernel(const ResArgs a, const PoolLaunch p) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    ResArgs v;
    if (!pool_res_view(a, p, v)) return;
    pool_resample_fast_role<kRes, kPoolResFastRows>(v, blockIdx.x, blockIdx.y, smem_raw);
}

// The slot-table resampler launch of all three sets: NR rows per workgroup, grid (tiles, row groups, slots); the
// free-form (kFast) or the reference-order kernel, interpolated or direct table.  `Set` names the set's kernels
// (set.fast<kRes, NR> / set.exact<kRes>) and appends its trailing arguments.  launch == false: the LDS check only.
template <class Set, bool kFast, int NR>
static bool launch_slot_resample(const Set &set, const ResArgs &a, const PoolLaunch &p, hipStream_t st, bool launch) {
    const size_t lds = (size_t)a.tab_bytes + sizeof(float) * (size_t)a.lds_floats * NR;
    if (lds > kMaxDynLds) return false;
    if (!launch || p.max_tiles <= 0) return true; // (max_tiles 0: dropped slices only, no output completed)
    census_resample(Set::census_set, kFast, a.interp != 0);
    census_resample_rung(Set::census_set, !kFast ? kResRungRef4 : NR == 2 ? kResRungVec2 : NR == 4 ? kResRungVec4 : kResRungVec8,
                         a.interp != 0, lds);
    const dim3 grid(p.max_tiles, (a.rows + NR - 1) / NR, p.nslots);
    if constexpr (kFast) {
        if (a.interp) set.template fast<2, NR>(grid, lds, st, a);
        else set.template fast<1, NR>(grid, lds, st, a);
    } else {
        if (a.interp) set.template exact<2>(grid, lds, st, a);
        else set.template exact<1>(grid, lds, st, a);
    }
    return true;
}

struct PoolResampleSet { // trailing argument p
    static constexpr int census_set = 1;
    const PoolLaunch &p;
    template <int kRes, int NR> void fast(dim3 grid, size_t lds, hipStream_t st, const ResArgs &a) const {
        static_assert(NR == kPoolResFastRows, "the kernel's row count");
        launch_big_lds<pv_pool_resample_fast_kernel<kRes>>(grid, dim3(kTileOut), lds, st, a, p);
    }
    template <int kRes> void exact(dim3 grid, size_t lds, hipStream_t st, const ResArgs &a) const {
        launch_big_lds<pv_pool_resample_kernel<kRes>>(grid, dim3(kTileOut), lds, st, a, p);
    }
};
bool launch_pool_resample(const ResArgs &a, const PoolLaunch &p, hipStream_t st, bool launch) {
    return a.fast ? launch_slot_resample<PoolResampleSet, true, kPoolResFastRows>({p}, a, p, st, launch)
                  : launch_slot_resample<PoolResampleSet, false, kResRows>({p}, a, p, st, launch);
}

// --------------------------------------------------------------------------------------------
// Stream pool with per-slot parameters (pv_kernels.h PoolParams): the per-slot kernels above, whose slot view also
// takes the slot's hop, phase advance, frequency compensation, gain and resampler set-up from its PoolParams entry.
// They call the same device functions with the same values a single-stream engine of the slot's configuration passes
// as launch-wide arguments, so a slot computes exactly what that engine computes.  The kernels above stay as they are.
// --------------------------------------------------------------------------------------------
template <int NC> __global__ __launch_bounds__(64) void pv_pmix_analyze_wave_kernel(const AnalyzeArgs a, const PoolLaunch p,
                                                                                   const PoolParams *__restrict__ q) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    const PoolSlot ps = p.slots[blockIdx.y];
    const int tl = __builtin_amdgcn_readfirstlane((int)blockIdx.x / a.rows), row = blockIdx.x - tl * a.rows;
    if (tl >= ps.Tn) return;
    AnalyzeArgs v = pool_view(a, ps);
    v.hop = q[blockIdx.y].hop;
    analyze_wave_role<NC, WF<NC>::LDS_CF * sizeof(cf)>(v, row, tl, reinterpret_cast<cf *>(smem_raw));
}
__global__ __launch_bounds__(128) void pv_pmix_analyze_split_kernel(const AnalyzeArgs a, const PoolLaunch p,
                                                                     const PoolParams *__restrict__ q) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    const PoolSlot ps = p.slots[blockIdx.y];
    const int tl = __builtin_amdgcn_readfirstlane((int)blockIdx.x / a.rows), row = blockIdx.x - tl * a.rows;
    if (tl >= ps.Tn) return;
    AnalyzeArgs v = pool_view(a, ps);
    v.hop = q[blockIdx.y].hop;
    analyze_split_role<WF2048S, WF2048S::LDS_CF * sizeof(cf)>(v, row, tl, reinterpret_cast<cf *>(smem_raw));
}

struct PmixAnalyzeSet { // trailing arguments p, q
    static constexpr int census_set = 2;
    const PoolLaunch &p;
    const PoolParams *q;
    template <int NC, bool kBigLds> void wave(dim3 grid, size_t lds, hipStream_t st, const AnalyzeArgs &a) const {
        launch_maybe_big_lds<pv_pmix_analyze_wave_kernel<NC>, kBigLds>(grid, dim3(64), lds, st, a, p, q);
    }
    void split(dim3 grid, size_t lds, hipStream_t st, const AnalyzeArgs &a) const {
        hipLaunchKernelGGL(pv_pmix_analyze_split_kernel, grid, dim3(WF2048S::LANES), lds, st, a, p, q);
    }
};
bool launch_pmix_analyze(const AnalyzeArgs &a, const PoolLaunch &p, const PoolParams *q, hipStream_t st) {
    return launch_slot_analyze(PmixAnalyzeSet{p, q}, a, p, st);
}

// phase-locked mode: match + rotation chain, one workgroup per (channel, slot)
template <int D>
__global__ __launch_bounds__(1024) void pv_pmix_phase_kernel(const MatchArgs m, const SeqArgs a, const PoolLaunch p,
                                                             const PoolParams *__restrict__ q) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    const PoolSlot ps = p.slots[blockIdx.y];
    const int hop = q[blockIdx.y].hop;
    const double two_pi_hop = q[blockIdx.y].two_pi_hop;
    const int64_t r = ps.row0;
    const int32_t *pinc = reinterpret_cast<const int32_t *>(p.desc + ps.pinc_off);
    MatchArgs mv = m;
    mv.hop = hop, mv.two_pi_hop = two_pi_hop;
    mv.t0 = ps.t0, mv.s0 = ps.s0, mv.Tn = ps.Tn, mv.phase_inc = pinc;
    mv.phase += r * m.TR * m.HP;
    mv.peaks += r * m.TR * m.PKP;
    mv.npk += r * m.TR;
    mv.recs += r * m.TR * m.PKP;
    mv.modes += r * m.TR;
    SeqArgs av = a;
    av.hop = hop, av.two_pi_hop = two_pi_hop;
    av.t0 = ps.t0, av.s0 = ps.s0, av.Tn = ps.Tn, av.phase_inc = pinc;
    av.phase = mv.phase, av.peaks = mv.peaks, av.npk = mv.npk, av.recs = mv.recs, av.modes = mv.modes;
    av.rot += r * a.TR * a.PKP;
    av.outphase += r * a.TR * a.HP;
    av.st_kind += r;
    av.st_rot += r * a.PKP;
    av.st_po += r * a.hs;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
    for (int tl = wave; tl < mv.Tn; tl += nw)
        match_wave_role(mv, blockIdx.x, tl, smem_raw + (size_t)wave * match_wave_lds(mv.hs, mv.PKP));
    __threadfence(); // the records go through global memory: the chain's loads must see them
    __syncthreads();
    if (av.high_prio) __builtin_amdgcn_s_setprio(3);
    seq_role_ring<D>(av, blockIdx.x, smem_raw);
}

bool launch_pmix_phase(const MatchArgs &m, const SeqArgs &a, const PoolLaunch &p, const PoolParams *q, hipStream_t st) {
    if (!pool_phase_supported(a.hs, a.PKP)) return false;
    census_phase(2, kPhaseFormFused, kPoolSeqDepth);
    launch_big_lds<pv_pmix_phase_kernel<kPoolSeqDepth>>(dim3(a.rows, p.nslots), dim3(seq_threads(a.PKP)),
                       pool_phase_lds(a.hs, a.PKP), st, m, a, p, q);
    return true;
}

// coremode 0: the per-bin recurrence; grid (bins / 256, C, slots)
__global__ __launch_bounds__(kPropThreads) void pv_pmix_prop_kernel(const PropArgs a, const PoolLaunch p,
                                                                    const PoolParams *__restrict__ q) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const PoolSlot ps = p.slots[blockIdx.z];
    const int64_t r = ps.row0;
    PropArgs v = a;
    v.hop = q[blockIdx.z].hop;
    v.two_pi_hop = q[blockIdx.z].two_pi_hop;
    v.t0 = ps.t0, v.s0 = ps.s0, v.Tn = ps.Tn;
    v.phase_inc = reinterpret_cast<const int32_t *>(p.desc + ps.pinc_off);
    v.phase += r * a.TR * a.HP;
    v.outphase += r * a.TR * a.HP;
    v.st_pp += r * a.hs;
    v.st_po += r * a.hs;
    if (i < a.hs) prop_role(v, blockIdx.y, i);
}

bool launch_pmix_prop(const PropArgs &a, const PoolLaunch &p, const PoolParams *q, hipStream_t st) {
    hipLaunchKernelGGL(pv_pmix_prop_kernel, dim3((a.hs + kPropThreads - 1) / kPropThreads, a.rows, p.nslots),
                       dim3(kPropThreads), 0, st, a, p, q);
    return true;
}

// fused synthesis + overlap-add: one workgroup per (channel, slot); the launch's slots share do_freq_comp, resample and
// fast (the variant), each brings its own hop, phase advance, frequency compensation and gain
template <int NC, int kPlainCore, int kRes, bool kFast>
__global__ __launch_bounds__(pool_chain_max_threads(NC, kPlainCore, kFast)) void pv_pmix_synth_chain_kernel(
    const SynthArgs s, const ChainArgs c, const PoolLaunch p, const PoolParams *__restrict__ q) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    const PoolSlot ps = p.slots[blockIdx.y];
    const PoolParams *__restrict__ qs = q + blockIdx.y;
    const int64_t r = ps.row0;
    SynthArgs sv = s;
    sv.hop = qs->hop;
    sv.two_pi_hop = qs->two_pi_hop;
    sv.do_freq_comp = qs->do_freq_comp;
    sv.freq_comp = qs->freq_comp;
    sv.fixed_gain = qs->fixed_gain;
    sv.t0 = ps.t0, sv.s0 = ps.s0, sv.Tn = ps.Tn;
    sv.phase_inc = reinterpret_cast<const int32_t *>(p.desc + ps.pinc_off);
    const int64_t plane = r * s.TR * s.tb.HP;
    sv.mag += plane;
    sv.phase += plane;
    if (sv.outphase) sv.outphase += plane;
    if (sv.peaks) sv.peaks += r * s.TR * s.PKP;
    if (sv.npk) sv.npk += r * s.TR;
    if (sv.modes) sv.modes += r * s.TR;
    if (sv.rot) sv.rot += r * s.TR * s.PKP;
    if constexpr (kPlainCore < 0) { // the voice setting: a whisper slot of a ROBOTIC object reads its drawn phases
        sv.whisper = (s.whisper && ps.wh_off >= 0) ? s.whisper + ps.wh_off : nullptr;
        if (sv.whisper) sv.robotic = 0;
        // the carrier setting: a carrier slot is a channel vocoder over its own carrier planes (band length as derive())
        if (s.cmag && ps.car_off >= 0) {
            sv.cmag = s.cmag + ps.car_off, sv.cphase = s.cphase + ps.car_off;
            sv.voc_band_len = (2 * NC) / 1024;
            sv.robotic = 0;
        }
    }
    ChainArgs cv = c;
    cv.Tn = ps.Tn;
    cv.t0 = ps.t0;
    cv.slices = reinterpret_cast<const ChainSlice *>(p.desc + ps.cs_off);
    cv.run_off = reinterpret_cast<const int32_t *>(p.desc + ps.ro_off);
    cv.wden = reinterpret_cast<const float *>(p.desc + ps.wden_off);
    cv.wden_hi = cv.wden;
    cv.st_acc += 2 * r * c.AR; // [slot][2][C][AR]
    cv.acc_sel = ps.acc_sel;
    if (kRes) cv.stream += r * ((int64_t)c.smask + 1);
    cv.out = p.out + ps.out_off;
    cv.out_stride_row = ps.out_stride_row;
    pool_synth_chain_role<NC, kPlainCore, kRes, kFast>(sv, cv, blockIdx.x, smem_raw);
}

struct PmixChainSet { // grid (rows, slots); trailing arguments p, q
    static constexpr int census_set = 2;
    const SynthArgs &s;
    const PoolLaunch &p;
    const PoolParams *q;
    hipStream_t st;
    static constexpr int max_threads(int NC, int kPlainCore, bool kFast) { return pool_chain_max_threads(NC, kPlainCore, kFast); }
    static bool fit_waves(ChainArgs &c, int max_threads) { return slot_chain_fit_waves(c, max_threads); }
    template <int NC, int kPlainCore, int kRes, bool kFast> void launch(const ChainArgs &c, dim3 block, size_t lds) const {
        launch_big_lds<pv_pmix_synth_chain_kernel<NC, kPlainCore, kRes, kFast>>(dim3(c.rows, p.nslots), block, lds, st, s, c, p, q);
    }
};
// (s.do_freq_comp: the launch's variant)
bool launch_pmix_synth_chain(const SynthArgs &s, const ChainArgs &c, const PoolLaunch &p, const PoolParams *q,
                             hipStream_t st, bool launch) {
    return launch_chain(PmixChainSet{s, p, q, st}, s, s.tb.nc, c, launch);
}

// resampling: grid (tiles, row groups, slots); the launch's slots share interp and fast
__device__ __forceinline__ bool pmix_res_view(const ResArgs &a, const PoolLaunch &p, const PoolParams *__restrict__ q,
                                              ResArgs &v) {
    if (!pool_res_view(a, p, v)) return false;
    const PoolParams *__restrict__ qs = q + blockIdx.z;
    v.filt_len = qs->filt_len;
    v.oversample = qs->oversample;
    v.sinc = qs->sinc;
    v.sinc_len = qs->sinc_len;
    v.tab4 = qs->tab4;
    v.tab_bytes = qs->tab_bytes;
    v.lds_floats = qs->lds_floats;
    return true;
}
template <int kRes>
__global__ __launch_bounds__(kTileOut) void pv_pmix_resample_kernel(const ResArgs a, const PoolLaunch p, const PoolParams *__restrict__ q) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    ResArgs v;
    if (!pmix_res_view(a, p, q, v)) return;
    pool_resample_role<kRes>(v, blockIdx.x, blockIdx.y, smem_raw);
}
template <int kRes>
__global__ __launch_bounds__(kTileOut) void pv_pmix_resample_fast_kernel(const ResArgs a, const PoolLaunch p,
                                                                         const PoolParams *__restrict__ q) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    ResArgs v;
    if (!pmix_res_view(a, p, q, v)) return;
    pool_resample_fast_role<kRes, kPoolResFastRows>(v, blockIdx.x, blockIdx.y, smem_raw);
}

struct PmixResampleSet { // trailing arguments p, q
    static constexpr int census_set = 2;
    const PoolLaunch &p;
    const PoolParams *q;
    template <int kRes, int NR> void fast(dim3 grid, size_t lds, hipStream_t st, const ResArgs &a) const {
        static_assert(NR == kPoolResFastRows, "the kernel's row count");
        launch_big_lds<pv_pmix_resample_fast_kernel<kRes>>(grid, dim3(kTileOut), lds, st, a, p, q);
    }
    template <int kRes> void exact(dim3 grid, size_t lds, hipStream_t st, const ResArgs &a) const {
        launch_big_lds<pv_pmix_resample_kernel<kRes>>(grid, dim3(kTileOut), lds, st, a, p, q);
    }
};
bool launch_pmix_resample(const ResArgs &a, const PoolLaunch &p, const PoolParams *q, hipStream_t st, bool launch) {
    return a.fast ? launch_slot_resample<PmixResampleSet, true, kPoolResFastRows>({p, q}, a, p, st, launch)
                  : launch_slot_resample<PmixResampleSet, false, kResRows>({p, q}, a, p, st, launch);
}

// --------------------------------------------------------------------------------------------
// Mixed batch (pv_kernels.h MbSlot): the batch path's long launches over a slot table.  The stages are the device
// functions the batch and pool kernels call, given the values a single-stream batch of the slot's configuration and
// length passes as launch-wide arguments, so a slot computes exactly what that batch computes.
// --------------------------------------------------------------------------------------------
// analysis: the slot's rows of the caller's packed input ([C][frames] at in_off, zeros from `frames` on), its hop
__device__ __forceinline__ AnalyzeArgs mb_view(const AnalyzeArgs &a, const PoolSlot &ps, const int hop, const MbSlot &ms) {
    AnalyzeArgs v = a;
    const int64_t r = ps.row0;
    v.t0 = ps.t0, v.s0 = ps.s0, v.Tn = ps.Tn;
    v.hop = hop;
    v.ia.in = a.ia.in + ms.in_off;
    v.ia.stride_c = ms.frames;
    v.ia.stride_s = 0;
    v.ia.mask = ~0ull;
    v.ia.len = ms.frames;
    v.mag += r * a.TR * a.tb.HP;
    v.phase += r * a.TR * a.tb.HP;
    if (a.find_peaks) {
        v.peaks += r * a.TR * a.PKP;
        v.npk += r * a.TR;
    }
    return v;
}
// one wave per frame: workgroup x = tl * C + c, y = slot
template <int NC> __global__ __launch_bounds__(64) void pv_mb_analyze_wave_kernel(const AnalyzeArgs a, const PoolLaunch p,
                                                                                 const PoolParams *__restrict__ q,
                                                                                 const MbSlot *__restrict__ m) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    const PoolSlot ps = p.slots[blockIdx.y];
    const int tl = __builtin_amdgcn_readfirstlane((int)blockIdx.x / a.rows), row = blockIdx.x - tl * a.rows;
    if (tl >= ps.Tn) return;
    analyze_wave_role<NC, WF<NC>::LDS_CF * sizeof(cf)>(mb_view(a, ps, q[blockIdx.y].hop, m[blockIdx.y]), row, tl,
                                                       reinterpret_cast<cf *>(smem_raw));
}
__global__ __launch_bounds__(128) void pv_mb_analyze_split_kernel(const AnalyzeArgs a, const PoolLaunch p,
                                                                   const PoolParams *__restrict__ q,
                                                                   const MbSlot *__restrict__ m) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    const PoolSlot ps = p.slots[blockIdx.y];
    const int tl = __builtin_amdgcn_readfirstlane((int)blockIdx.x / a.rows), row = blockIdx.x - tl * a.rows;
    if (tl >= ps.Tn) return;
    analyze_split_role<WF2048S, WF2048S::LDS_CF * sizeof(cf)>(mb_view(a, ps, q[blockIdx.y].hop, m[blockIdx.y]), row, tl,
                                                              reinterpret_cast<cf *>(smem_raw));
}

struct MbAnalyzeSet { // trailing arguments p, q, m
    static constexpr int census_set = 3;
    const PoolLaunch &p;
    const PoolParams *q;
    const MbSlot *m;
    template <int NC, bool kBigLds> void wave(dim3 grid, size_t lds, hipStream_t st, const AnalyzeArgs &a) const {
        launch_maybe_big_lds<pv_mb_analyze_wave_kernel<NC>, kBigLds>(grid, dim3(64), lds, st, a, p, q, m);
    }
    void split(dim3 grid, size_t lds, hipStream_t st, const AnalyzeArgs &a) const {
        hipLaunchKernelGGL(pv_mb_analyze_split_kernel, grid, dim3(WF2048S::LANES), lds, st, a, p, q, m);
    }
};
bool launch_mb_analyze(const AnalyzeArgs &a, const PoolLaunch &p, const PoolParams *q, const MbSlot *m, hipStream_t st) {
    return launch_slot_analyze(MbAnalyzeSet{p, q, m}, a, p, st);
}

// phase-locked mode, parallel part: four waves, one step of the slot each; grid (steps / 4, C, slots)
__global__ __launch_bounds__(kMatchThreads) void pv_mb_match_kernel(const MatchArgs m, const PoolLaunch p,
                                                                    const PoolParams *__restrict__ q) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    const PoolSlot ps = p.slots[blockIdx.z];
    const int wave = threadIdx.x >> 6;
    const int tl = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave);
    if (tl >= ps.Tn) return; // wave-uniform
    const int64_t r = ps.row0;
    MatchArgs mv = m;
    mv.hop = q[blockIdx.z].hop, mv.two_pi_hop = q[blockIdx.z].two_pi_hop;
    mv.t0 = ps.t0, mv.s0 = ps.s0, mv.Tn = ps.Tn;
    mv.phase_inc = reinterpret_cast<const int32_t *>(p.desc + ps.pinc_off);
    mv.phase += r * m.TR * m.HP;
    mv.peaks += r * m.TR * m.PKP;
    mv.npk += r * m.TR;
    mv.recs += r * m.TR * m.PKP;
    mv.modes += r * m.TR;
    match_wave_role(mv, blockIdx.y, tl, smem_raw + (size_t)wave * match_wave_lds(mv.hs, mv.PKP));
}
bool launch_mb_match(const MatchArgs &a, const PoolLaunch &p, const PoolParams *q, hipStream_t st) {
    const size_t lds = 4 * match_wave_lds(a.hs, a.PKP);
    hipLaunchKernelGGL(pv_mb_match_kernel, dim3((p.max_tn + 3) / 4, a.rows, p.nslots), dim3(kMatchThreads), lds, st, a, p, q);
    return true;
}

// ... and the rotation chain: one workgroup per (channel, slot) walks the slot's steps of the launch
constexpr int kMbSeqDepth = 4; // (launch_seq: four steps ahead where the chain shares its CUs with other rows' workgroups)
template <int D>
__global__ __launch_bounds__(1024) void pv_mb_seq_kernel(const SeqArgs a, const PoolLaunch p, const PoolParams *__restrict__ q) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    const PoolSlot ps = p.slots[blockIdx.y];
    const int64_t r = ps.row0;
    SeqArgs av = a;
    av.hop = q[blockIdx.y].hop, av.two_pi_hop = q[blockIdx.y].two_pi_hop;
    av.t0 = ps.t0, av.s0 = ps.s0, av.Tn = ps.Tn;
    av.phase_inc = reinterpret_cast<const int32_t *>(p.desc + ps.pinc_off);
    av.phase += r * a.TR * a.HP;
    av.peaks += r * a.TR * a.PKP;
    av.npk += r * a.TR;
    av.recs += r * a.TR * a.PKP;
    av.modes += r * a.TR;
    av.rot += r * a.TR * a.PKP;
    av.outphase += r * a.TR * a.HP;
    av.st_kind += r;
    av.st_rot += r * a.PKP;
    av.st_po += r * a.hs;
    if (av.high_prio) __builtin_amdgcn_s_setprio(3);
    seq_role_ring<D>(av, blockIdx.x, smem_raw);
}
static size_t mb_seq_lds(const SeqArgs &a) {
    return ((seq_lds_bytes(a) + 15) & ~(size_t)15) + (size_t)kMbSeqDepth * seq_threads(a.PKP) * sizeof(PeakRec);
}
bool launch_mb_seq(const SeqArgs &a, const PoolLaunch &p, const PoolParams *q, hipStream_t st) {
    if (a.PKP > seq_threads(a.PKP) || mb_seq_lds(a) > kMaxDynLds) return false;
    census_phase(3, kPhaseFormRing, kMbSeqDepth);
    launch_big_lds<pv_mb_seq_kernel<kMbSeqDepth>>(dim3(a.rows, p.nslots), dim3(seq_threads(a.PKP)), mb_seq_lds(a), st, a, p, q);
    return true;
}

// fused synthesis + overlap-add: one workgroup per (channel, run, slot).  The launch's slots share do_freq_comp,
// resample and fast (the variant); each brings its own hop, phase advance, frequency compensation, gain and run lists.
// Run 0 of a slot reads the slot's carried accumulator half, its last run writes the other one (ChainArgs::acc_sel,
// per slot: PoolSlot::acc_sel), so no run of one launch can overwrite what another run of it still has to read.
template <int NC, int kPlainCore, int kRes, bool kFast>
__global__ __launch_bounds__(pool_chain_max_threads(NC, kPlainCore, kFast)) void pv_mb_synth_chain_kernel(
    const SynthArgs s, const ChainArgs c, const PoolLaunch p, const PoolParams *__restrict__ q, const MbSlot *__restrict__ m) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    const int runs = m[blockIdx.z].runs, run = blockIdx.y;
    if (run >= runs) return; // workgroup-uniform
    const PoolSlot ps = p.slots[blockIdx.z];
    const PoolParams *__restrict__ qs = q + blockIdx.z;
    const int64_t r = ps.row0;
    SynthArgs sv = s;
    sv.hop = qs->hop;
    sv.two_pi_hop = qs->two_pi_hop;
    sv.do_freq_comp = qs->do_freq_comp;
    sv.freq_comp = qs->freq_comp;
    sv.fixed_gain = qs->fixed_gain;
    sv.t0 = ps.t0, sv.s0 = ps.s0, sv.Tn = ps.Tn;
    sv.phase_inc = reinterpret_cast<const int32_t *>(p.desc + ps.pinc_off);
    const int64_t plane = r * s.TR * s.tb.HP;
    sv.mag += plane;
    sv.phase += plane;
    if (sv.outphase) sv.outphase += plane;
    if (sv.peaks) sv.peaks += r * s.TR * s.PKP;
    if (sv.npk) sv.npk += r * s.TR;
    if (sv.modes) sv.modes += r * s.TR;
    if (sv.rot) sv.rot += r * s.TR * s.PKP;
    if constexpr (kPlainCore < 0) { // the voice setting: a whisper slot of a ROBOTIC object reads its drawn phases
        sv.whisper = (s.whisper && ps.wh_off >= 0) ? s.whisper + ps.wh_off : nullptr;
        if (sv.whisper) sv.robotic = 0;
    }
    ChainArgs cv = c;
    cv.Tn = ps.Tn;
    cv.t0 = ps.t0;
    cv.runs = runs;
    cv.slices = reinterpret_cast<const ChainSlice *>(p.desc + ps.cs_off);
    cv.run_off = reinterpret_cast<const int32_t *>(p.desc + ps.ro_off);
    cv.wden = reinterpret_cast<const float *>(p.desc + ps.wden_off);
    cv.wden_hi = cv.wden;
    cv.st_acc += 2 * r * c.AR; // [slot][2][C][AR]
    cv.acc_sel = ps.acc_sel;
    if (kRes) cv.stream += r * ((int64_t)c.smask + 1);
    cv.out = p.out + ps.out_off;
    cv.out_stride_row = ps.out_stride_row;
    pool_synth_chain_role<NC, kPlainCore, kRes, kFast>(sv, cv, blockIdx.x, smem_raw, run, run == runs - 1);
}

struct MbChainSet { // grid (rows, max_runs, slots); trailing arguments p, q, m
    static constexpr int census_set = 3;
    const SynthArgs &s;
    const PoolLaunch &p;
    const PoolParams *q;
    const MbSlot *m;
    int max_runs;
    hipStream_t st;
    static constexpr int max_threads(int NC, int kPlainCore, bool kFast) { return pool_chain_max_threads(NC, kPlainCore, kFast); }
    static bool fit_waves(ChainArgs &c, int max_threads) { return slot_chain_fit_waves(c, max_threads); }
    template <int NC, int kPlainCore, int kRes, bool kFast> void launch(const ChainArgs &c, dim3 block, size_t lds) const {
        launch_big_lds<pv_mb_synth_chain_kernel<NC, kPlainCore, kRes, kFast>>(dim3(c.rows, max_runs, p.nslots), block, lds, st, s, c,
                                                                              p, q, m);
    }
};
// (s.do_freq_comp: the launch's variant)
bool launch_mb_synth_chain(const SynthArgs &s, const ChainArgs &c, const PoolLaunch &p, const PoolParams *q, const MbSlot *m,
                           int max_runs, hipStream_t st, bool launch) {
    if (max_runs < 1 || max_runs > 65535) return false; // (the grid's y)
    return launch_chain(MbChainSet{s, p, q, m, max_runs, st}, s, s.tb.nc, c, launch);
}

// resampling: grid (tiles, row groups, slots).  The pool's free-form kernel computes eight rows per workgroup, the
// missing ones of a slot with fewer channels included (computed, never stored); here a slot's C rows are all a
// workgroup ever has, so the row count is matched to them.  A row's sum does not depend on the rows beside it.
template <int kRes, int NR>
__global__ __launch_bounds__(kTileOut) void pv_mb_resample_fast_kernel(const ResArgs a, const PoolLaunch p,
                                                                       const PoolParams *__restrict__ q) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    PV_POISON_LDS(reinterpret_cast<char *>(smem_raw));
    ResArgs v;
    if (!pmix_res_view(a, p, q, v)) return;
    pool_resample_fast_role<kRes, NR>(v, blockIdx.x, blockIdx.y, smem_raw);
}
struct MbResampleSet { // trailing arguments p, q; the free-form kernel only
    static constexpr int census_set = 3;
    const PoolLaunch &p;
    const PoolParams *q;
    template <int kRes, int NR> void fast(dim3 grid, size_t lds, hipStream_t st, const ResArgs &a) const {
        launch_big_lds<pv_mb_resample_fast_kernel<kRes, NR>>(grid, dim3(kTileOut), lds, st, a, p, q);
    }
};
bool launch_mb_resample(const ResArgs &a, const PoolLaunch &p, const PoolParams *q, hipStream_t st, bool launch) {
    if (!a.fast) return launch_pmix_resample(a, p, q, st, launch); // the reference's order: four rows per workgroup
    if (a.rows <= 2) return launch_slot_resample<MbResampleSet, true, 2>({p, q}, a, p, st, launch);
    if (a.rows <= 4) return launch_slot_resample<MbResampleSet, true, 4>({p, q}, a, p, st, launch);
    return launch_slot_resample<MbResampleSet, true, kPoolResFastRows>({p, q}, a, p, st, launch);
}

// ---------------------------------------------------------------------------------------------------------------
// Mixed batch, descriptor build on the device (pv_mbatch_redraw): the two per-sample arrays of a stream's descriptors,
// written in the layout the stage kernels above read, from the per-slice records the host keeps.  One launch serves
// every (stream, group): block b belongs to the last job whose first_block is at or before it.  A lane writes 16
// bytes, neighbouring lanes neighbouring addresses.
// ---------------------------------------------------------------------------------------------------------------
constexpr int kMbBuildThreads = 256;
template <typename Job> __device__ __forceinline__ const Job &mb_build_job(const Job *__restrict__ jobs, int njobs) {
    int lo = 0, hi = njobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].first_block <= (int)blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    return jobs[lo];
}

// The window-sum denominators, as ChainBuilder::add / ChainBuilder::denominator (pv_engine.cc) compute them: sample n,
// finalised by slice t, starts at 1 (n == 0) or 0 and adds window[n - P_j] * win_gain for every slice j <= t whose
// frame covers it, oldest first; product and sum are rounded separately (this file is compiled with
// -ffp-contract=off, as the host's is; the pragma says so again where it matters).  A lane writes one ring quad, which
// lies within one slice: every slice's entries start on a 16-byte boundary.
__global__ __launch_bounds__(kMbBuildThreads) void pv_mb_build_wden_kernel(const MbWdenJob *__restrict__ jobs, int njobs,
                                                                           char *__restrict__ desc,
                                                                           const float *__restrict__ window) {
#pragma clang fp contract(off)
    const MbWdenJob &jb = mb_build_job(jobs, njobs);
    const int e0 = 4 * (((int)blockIdx.x - jb.first_block) * kMbBuildThreads + (int)threadIdx.x);
    if (e0 >= jb.total) return;
    const int64_t *__restrict__ P = reinterpret_cast<const int64_t *>(desc + jb.p_off);
    const int32_t *__restrict__ adv = reinterpret_cast<const int32_t *>(desc + jb.adv_off);
    const int32_t *__restrict__ wl = reinterpret_cast<const int32_t *>(desc + jb.woff_off); // wden_off | lead
    int a = 0, b = jb.Tn - 1; // the last slice of the group that starts at or before the quad (an empty one never wins)
    while (a < b) {
        const int mid = (a + b + 1) >> 1;
        if ((wl[jb.t0 + mid] & ~3) <= e0) a = mid;
        else b = mid - 1;
    }
    const int64_t t = (int64_t)jb.t0 + a;
    const int w = wl[t], av = adv[t], N = jb.N;
    const int i0 = e0 - (w & ~3) - (w & 3); // entry 0 of the slice belongs to sample P_t - lead
    const int64_t Pt = P[t];
    const float g = jb.win_gain;
    float acc[4];
    bool in[4], any = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        in[j] = i0 + j >= 0 && i0 + j < av;
        any = any || in[j];
        acc[j] = Pt + i0 + j == 0 ? 1.f : 0.f;
    }
    if (any) {
        int64_t jlo = t; // P never decreases: no slice before the first one that reaches the quad can cover it
        while (jlo > 0 && P[jlo - 1] + N > Pt + i0) --jlo;
        for (int64_t s = jlo; s <= t; ++s) {
            const int64_t off0 = Pt + i0 - P[s];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t off = off0 + j;
                if (in[j] && off >= 0 && off < N) {
                    const float term = window[off] * g;
                    acc[j] = acc[j] + term;
                }
            }
        }
    }
    float4 v;
    v.x = in[0] ? acc[0] : 1.f, v.y = in[1] ? acc[1] : 1.f, v.z = in[2] ? acc[2] : 1.f, v.w = in[3] ? acc[3] : 1.f;
    if (jb.fast) v.x = 1.0f / v.x, v.y = 1.0f / v.y, v.z = 1.0f / v.z, v.w = 1.0f / v.w; // IEEE division, as the host's
    *reinterpret_cast<float4 *>(desc + jb.dst_off + (int64_t)e0 * 4) = v;
}

// The resampler's output table, as build_res_tiles_of (pv_engine.cc) computes it, in 64-bit arithmetic (the host has
// checked that the stream's largest k * res_num fits).  A lane writes two entries of one tile.
__global__ __launch_bounds__(kMbBuildThreads) void pv_mb_build_otab_kernel(const MbOtabJob *__restrict__ jobs, int njobs,
                                                                           char *__restrict__ desc) {
    const MbOtabJob &jb = mb_build_job(jobs, njobs);
    const int64_t e0 = 2 * (((int64_t)blockIdx.x - jb.first_block) * kMbBuildThreads + (int64_t)threadIdx.x);
    if (e0 >= (int64_t)jb.ntiles * kTileOut) return;
    const int64_t k0 = jb.ka + (e0 / kTileOut) * kTileOut;
    const int o = (int)(e0 % kTileOut);
    const int kcnt = (int)((jb.kb - k0) < kTileOut ? (jb.kb - k0) : kTileOut);
    const uint64_t num = jb.res_num, den = jb.res_den;
    const uint64_t q0 = ((uint64_t)k0 * num) / den; // n_lo = filt_len / 2 + q0 - filt_len + 1
    uint32_t r[4];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        r[2 * j] = 0u, r[2 * j + 1] = 0u;
        if (o + j >= kcnt) continue;
        const uint64_t tot = (uint64_t)(k0 + o + j) * num;
        const uint64_t q = tot / den;
        const uint32_t frac_num = (uint32_t)(tot - q * den);
        const uint32_t xoff = (uint32_t)(q - q0);
        uint32_t sub, fbits = 0;
        if (jb.interp) {
            const uint32_t ov = (uint32_t)jb.oversample;
            sub = frac_num * ov / jb.res_den;
            const float frac = ((float)((frac_num * ov) % jb.res_den)) / (float)jb.res_den;
            fbits = __float_as_uint(frac);
        } else {
            sub = frac_num;
        }
        r[2 * j] = xoff | (sub << 16);
        r[2 * j + 1] = fbits;
    }
    *reinterpret_cast<uint4 *>(desc + jb.dst_off + e0 * (int64_t)sizeof(uint2)) = make_uint4(r[0], r[1], r[2], r[3]);
}

void launch_mb_build_wden(const MbWdenJob *jobs, int njobs, int nblocks, char *desc, const float *window, hipStream_t st) {
    if (njobs <= 0 || nblocks <= 0) return;
    hipLaunchKernelGGL(pv_mb_build_wden_kernel, dim3(nblocks), dim3(kMbBuildThreads), 0, st, jobs, njobs, desc, window);
}
void launch_mb_build_otab(const MbOtabJob *jobs, int njobs, int nblocks, char *desc, hipStream_t st) {
    if (njobs <= 0 || nblocks <= 0) return;
    hipLaunchKernelGGL(pv_mb_build_otab_kernel, dim3(nblocks), dim3(kMbBuildThreads), 0, st, jobs, njobs, desc);
}
int mb_build_wden_blocks(int total) { return (total / 4 + kMbBuildThreads - 1) / kMbBuildThreads; }
int mb_build_otab_blocks(int ntiles) { return (int)(((int64_t)ntiles * kTileOut / 2 + kMbBuildThreads - 1) / kMbBuildThreads); }

// ---------------------------------------------------------------------------------------------------------------
// Mixed batch, PCM wire (pv_mbatch_run_pcm): clip i's interleaved little-endian [frames][C] of 8 / 16 / 24 / 32 bits
// to its planar float [C][frames], and planar float to interleaved int16, with pv_pcm.h's conversions.  One launch
// each way serves every clip: block b belongs to the last job whose first_block is at or before it (mb_build_job)
// and moves one tile of kMbPcmTile interleaved samples, counted from the clip's start, through the LDS.
//   PCM side: a clip starts on a 16-byte boundary and a tile is a whole number of 16-sample groups (one, two, three
//   or four 16-byte pieces at 8 / 16 / 24 / 32 bits), so every tile starts on a sample and on a 16-byte boundary: a
//   lane moves one piece, neighbouring lanes neighbouring pieces.  Only what is left of a clip's last tile after its
//   last whole piece goes byte by byte (ingest) or sample by sample (egress); the padding behind it is neither read
//   nor written.
//   Planar side: the tile's samples of channel c are frames [f_lo, f_hi) of row c, which starts wherever the tight
//   packing puts it.  Lanes walk a row: single floats up to the first 16-byte boundary, float4 from there, single
//   floats for the rest (as pv_pool_snapshot_kernel: wide only where address and length allow).
// The transposition is the LDS index: the tile lies there in interleaved order (raw bytes on the way in, int16 on the
// way out), sample (f, c) at f * C + c - s0; with an odd C a frame straddles pieces and tiles, which this never sees.
// ---------------------------------------------------------------------------------------------------------------
constexpr int kMbPcmThreads = 256;
constexpr int kMbPcmTile = 4096;
static_assert(kMbPcmTile % 16 == 0, "a tile is whole 16-sample groups");

// frames f with f * C + c < x, for x in [0, frames * C]
__device__ __forceinline__ int64_t mb_pcm_rows_below(int64_t x, int c, int C) { return x <= c ? 0 : (x - c + C - 1) / C; }

template <int BPS> __device__ __forceinline__ float mb_pcm_lds_load(const unsigned char *raw, int idx) {
    if (BPS == 1) return pv_pcm_u8_to_f32(raw[idx]);
    if (BPS == 2) return pv_pcm_i16_to_f32((int16_t)reinterpret_cast<const uint16_t *>(raw)[idx]);
    if (BPS == 4) return pv_pcm_i32_to_f32((int32_t)reinterpret_cast<const uint32_t *>(raw)[idx]);
    return pv_pcm_load(raw + 3 * idx, 3);
}

// the planar side of one ingest tile: samples [s0, s0 + ns) of the clip, lying in `raw`
template <int BPS>
__device__ __forceinline__ void mb_pcm_ingest_rows(const unsigned char *raw, float *__restrict__ dst, const int64_t frames,
                                                   const int C, const int64_t s0, const int ns) {
    const int tid = (int)threadIdx.x;
    for (int c = 0; c < C; ++c) {
        const int64_t f_lo = mb_pcm_rows_below(s0, c, C), f_hi = mb_pcm_rows_below(s0 + ns, c, C);
        const int n = (int)(f_hi - f_lo);
        if (n <= 0) continue;
        float *__restrict__ row = dst + (int64_t)c * frames + f_lo;
        const int l0 = (int)(f_lo * C + c - s0);
        int head = (int)((0 - ((uintptr_t)row >> 2)) & 3);
        head = head < n ? head : n;
        const int quads = (n - head) >> 2;
        if (tid < head) row[tid] = mb_pcm_lds_load<BPS>(raw, l0 + tid * C);
        for (int q = tid; q < quads; q += kMbPcmThreads) {
            const int i = head + 4 * q, l = l0 + i * C;
            float4 v;
            v.x = mb_pcm_lds_load<BPS>(raw, l), v.y = mb_pcm_lds_load<BPS>(raw, l + C);
            v.z = mb_pcm_lds_load<BPS>(raw, l + 2 * C), v.w = mb_pcm_lds_load<BPS>(raw, l + 3 * C);
            *reinterpret_cast<float4 *>(row + i) = v;
        }
        const int i = head + 4 * quads + tid;
        if (i < n) row[i] = mb_pcm_lds_load<BPS>(raw, l0 + i * C);
    }
}

__global__ __launch_bounds__(kMbPcmThreads) void pv_mb_pcm_ingest_kernel(const MbPcmJob *__restrict__ jobs, int njobs,
                                                                        const unsigned char *__restrict__ pcm,
                                                                        float *__restrict__ planar) {
    __shared__ __attribute__((aligned(16))) unsigned char raw[kMbPcmTile * 4];
    const MbPcmJob jb = mb_build_job(jobs, njobs);
    const int C = jb.channels, bps = jb.bps, tid = (int)threadIdx.x;
    const int64_t total = jb.frames * C;
    const int64_t s0 = ((int64_t)blockIdx.x - jb.first_block) * kMbPcmTile;
    if (s0 >= total) return;
    const int ns = (int)(total - s0 < kMbPcmTile ? total - s0 : kMbPcmTile), nbytes = ns * bps;
    const unsigned char *__restrict__ src = pcm + jb.pcm_off + s0 * bps;
    const int pieces = nbytes >> 4;
    for (int p = tid; p < pieces; p += kMbPcmThreads)
        reinterpret_cast<uint4 *>(raw)[p] = reinterpret_cast<const uint4 *>(src)[p];
    for (int b = (pieces << 4) + tid; b < nbytes; b += kMbPcmThreads) raw[b] = src[b]; // (fewer than 16 bytes)
    __syncthreads();
    float *__restrict__ dst = planar + jb.planar_off;
    if (bps == 2) mb_pcm_ingest_rows<2>(raw, dst, jb.frames, C, s0, ns);
    else if (bps == 3) mb_pcm_ingest_rows<3>(raw, dst, jb.frames, C, s0, ns);
    else if (bps == 4) mb_pcm_ingest_rows<4>(raw, dst, jb.frames, C, s0, ns);
    else mb_pcm_ingest_rows<1>(raw, dst, jb.frames, C, s0, ns);
}

__global__ __launch_bounds__(kMbPcmThreads) void pv_mb_pcm_egress_kernel(const MbPcmJob *__restrict__ jobs, int njobs,
                                                                        const float *__restrict__ planar,
                                                                        unsigned char *__restrict__ pcm) {
    __shared__ __attribute__((aligned(16))) int16_t buf[kMbPcmTile];
    const MbPcmJob jb = mb_build_job(jobs, njobs);
    const int C = jb.channels, tid = (int)threadIdx.x;
    const int64_t total = jb.frames * C;
    const int64_t s0 = ((int64_t)blockIdx.x - jb.first_block) * kMbPcmTile;
    if (s0 >= total) return;
    const int ns = (int)(total - s0 < kMbPcmTile ? total - s0 : kMbPcmTile);
    const float *__restrict__ src = planar + jb.planar_off;
    for (int c = 0; c < C; ++c) {
        const int64_t f_lo = mb_pcm_rows_below(s0, c, C), f_hi = mb_pcm_rows_below(s0 + ns, c, C);
        const int n = (int)(f_hi - f_lo);
        if (n <= 0) continue;
        const float *__restrict__ row = src + (int64_t)c * jb.frames + f_lo;
        const int l0 = (int)(f_lo * C + c - s0);
        int head = (int)((0 - ((uintptr_t)row >> 2)) & 3);
        head = head < n ? head : n;
        const int quads = (n - head) >> 2;
        if (tid < head) buf[l0 + tid * C] = pv_pcm_f32_to_i16(row[tid]);
        for (int q = tid; q < quads; q += kMbPcmThreads) {
            const int i = head + 4 * q, l = l0 + i * C;
            const float4 v = *reinterpret_cast<const float4 *>(row + i);
            buf[l] = pv_pcm_f32_to_i16(v.x), buf[l + C] = pv_pcm_f32_to_i16(v.y);
            buf[l + 2 * C] = pv_pcm_f32_to_i16(v.z), buf[l + 3 * C] = pv_pcm_f32_to_i16(v.w);
        }
        const int i = head + 4 * quads + tid;
        if (i < n) buf[l0 + i * C] = pv_pcm_f32_to_i16(row[i]);
    }
    __syncthreads();
    unsigned char *__restrict__ dst = pcm + jb.pcm_off + s0 * 2;
    const int pieces = ns >> 3;
    for (int p = tid; p < pieces; p += kMbPcmThreads)
        reinterpret_cast<uint4 *>(dst)[p] = reinterpret_cast<const uint4 *>(buf)[p];
    const int s = (pieces << 3) + tid; // (fewer than 8 samples)
    if (s < ns) reinterpret_cast<int16_t *>(dst)[s] = buf[s];
}

int64_t mb_pcm_blocks(int64_t frames, int channels) { return (frames * channels + kMbPcmTile - 1) / kMbPcmTile; }
void launch_mb_pcm_ingest(const MbPcmJob *jobs, int njobs, int nblocks, const void *pcm, float *planar, hipStream_t st) {
    if (njobs <= 0 || nblocks <= 0) return;
    hipLaunchKernelGGL(pv_mb_pcm_ingest_kernel, dim3(nblocks), dim3(kMbPcmThreads), 0, st, jobs, njobs,
                       static_cast<const unsigned char *>(pcm), planar);
}
void launch_mb_pcm_egress(const MbPcmJob *jobs, int njobs, int nblocks, const float *planar, void *pcm, hipStream_t st) {
    if (njobs <= 0 || nblocks <= 0) return;
    hipLaunchKernelGGL(pv_mb_pcm_egress_kernel, dim3(nblocks), dim3(kMbPcmThreads), 0, st, jobs, njobs, planar,
                       static_cast<unsigned char *>(pcm));
}

} // namespace pv
