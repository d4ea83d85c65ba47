// pv_hostio.hip -- the batch engine with the host staging included (include/audiomod_pv.h, pv_hostio_*).
//
// The reference's callers keep their audio in host memory: planar float buffers per channel, filled from and
// written to 16-bit WAV data (main/main.cc:152-162,484-491; main/wavfile.cc:733-755,1334-1342).  Here `nstreams`
// such streams are processed in groups; a group's host-to-device copy, its kernels (pv_batch_run) and its
// device-to-host copy run on three HIP streams, so that while group g computes, group g+1 arrives and group g-1
// leaves.  With int16 on the wire the conversions of the reference's WAV reader and writer run on the device.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "audiomod_pv.h"
#include "pv_atan2f.h"
#include "pv_plan.h"
#include "pv_wire.h"

namespace {

// main/wavfile.cc:733-755: float = (float)(int16 * (1.0 / 32768.0)) -- exact, so one float multiply gives the same
__global__ void pv_i16_to_f32(const int16_t *__restrict__ in, float *__restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (float)in[i] * (1.0f / 32768.0f);
}
// main/wavfile.cc:1295-1306,1334-1342: (short)saturate(x * 32768.0f, -32768.0f, 32767.0f), truncation toward zero
__global__ void pv_f32_to_i16(const float *__restrict__ in, int16_t *__restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float v = in[i] * 32768.0f;
    if (v > 32767.0f) v = 32767.0f;
    else if (v < -32768.0f) v = -32768.0f;
    out[i] = (int16_t)(int)v;
}

// The same two conversions on row windows (the segmented object's slots): `rows` rows of `width` valid samples, both
// arrays with a row pitch of `pitch` samples, a multiple of 8, on 16-byte-aligned bases -- so every row of either
// type starts on a 16-byte boundary.  A lane takes eight consecutive samples: one 16-byte access on the int16 side
// (lanes 16 bytes apart: a wave instruction covers whole cache lines), two on the float side (lanes 32 bytes apart:
// each of the two instructions covers half of every line the wave touches, the other covers the rest right behind it).
// The last, partial eight of a row go sample by sample.  A row takes bpr = ceil(width / 2048) workgroups; the grid is
// one-dimensional (rows x bpr workgroups), so the row count is not bound by the 65 535 of a grid's second dimension.
// The expressions are the flat kernels' (pv_wire.h: shared with the stream pool's ingest and egress kernels).
__global__ __launch_bounds__(256) void pv_rows_i16_to_f32(const int16_t *__restrict__ in, float *__restrict__ out,
                                                          int rows, int64_t width, int64_t pitch, unsigned bpr) {
    const int row = (int)(blockIdx.x / bpr);
    const int64_t i8 = ((int64_t)(blockIdx.x % bpr) * blockDim.x + threadIdx.x) * 8;
    if (row >= rows || i8 >= width) return;
    const int16_t *__restrict__ src = in + (int64_t)row * pitch + i8;
    float *__restrict__ dst = out + (int64_t)row * pitch + i8;
    if (i8 + 8 <= width) {
        const uint4 w = *reinterpret_cast<const uint4 *>(src);
        const uint32_t u[4] = {w.x, w.y, w.z, w.w};
        float f[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f[2 * j] = pv_wire_i16_to_f32((int16_t)(uint16_t)(u[j] & 0xffffu));
            f[2 * j + 1] = pv_wire_i16_to_f32((int16_t)(uint16_t)(u[j] >> 16));
        }
        reinterpret_cast<float4 *>(dst)[0] = make_float4(f[0], f[1], f[2], f[3]);
        reinterpret_cast<float4 *>(dst)[1] = make_float4(f[4], f[5], f[6], f[7]);
    } else {
        for (int j = 0; i8 + j < width; ++j) dst[j] = pv_wire_i16_to_f32(src[j]);
    }
}
__global__ __launch_bounds__(256) void pv_rows_f32_to_i16(const float *__restrict__ in, int16_t *__restrict__ out,
                                                          int rows, int64_t width, int64_t pitch, unsigned bpr) {
    const int row = (int)(blockIdx.x / bpr);
    const int64_t i8 = ((int64_t)(blockIdx.x % bpr) * blockDim.x + threadIdx.x) * 8;
    if (row >= rows || i8 >= width) return;
    const float *__restrict__ src = in + (int64_t)row * pitch + i8;
    int16_t *__restrict__ dst = out + (int64_t)row * pitch + i8;
    if (i8 + 8 <= width) {
        const float4 a = reinterpret_cast<const float4 *>(src)[0], b = reinterpret_cast<const float4 *>(src)[1];
        const float f[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        uint32_t u[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            u[j] = (uint32_t)(uint16_t)pv_wire_f32_to_i16(f[2 * j]) | ((uint32_t)(uint16_t)pv_wire_f32_to_i16(f[2 * j + 1]) << 16);
        *reinterpret_cast<uint4 *>(dst) = make_uint4(u[0], u[1], u[2], u[3]);
    } else {
        for (int j = 0; i8 + j < width; ++j) dst[j] = pv_wire_f32_to_i16(src[j]);
    }
}

// the analysis kernels' atan2f (pv_atan2f.h, device build: short division) on arrays, for pv_debug_atan2f
__global__ void pv_atan2f_probe(const float *__restrict__ y, const float *__restrict__ x, float *__restrict__ out,
                                int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = pv_atan2f_fd_finite(y[i], x[i]);
}

// ... and the wave-per-frame kernels' polar conversion (table-driven atan2f, range-tested short division and square
// root, IEEE operations otherwise: pv_kernels.hip analyze_wave_role), for pv_debug_polar
__device__ const PvAtanBlob pv_atan_blob_probe = pv_atan_make_blob();
__global__ void pv_polar_probe(const float *__restrict__ im, const float *__restrict__ re, float *__restrict__ ph,
                               float *__restrict__ mag, int64_t n) {
    __shared__ __attribute__((aligned(16))) uint32_t tab[PV_ATAN_BLOB_WORDS];
    if (threadIdx.x < PV_ATAN_BLOB_WORDS) tab[threadIdx.x] = pv_atan_blob_probe.w[threadIdx.x];
    __syncthreads();
    typedef __attribute__((address_space(3))) const unsigned char lds_u8;
    const unsigned char *atab = reinterpret_cast<const unsigned char *>((uintptr_t)(lds_u8 *)tab); // LDS address as a number
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float y = im[i], x = re[i];
    const float a = x * x + y * y;
    const float mx = fmaxf(fabsf(x), fabsf(y)), mn = fminf(fabsf(x), fabsf(y));
    if (mx < 0x1p63f && mn >= 0x1p-48f) {
        mag[i] = pv_sqrt_safe(a);
        ph[i] = pv_atan2f_fd_tab<true>(y, x, atab);
    } else {
        mag[i] = sqrtf(a);
        ph[i] = pv_atan2f_fd_tab<false>(y, x, atab);
    }
}

// every float with bit pattern in [first, first + count): pv_sqrt_safe against the compiler's correctly rounded sqrtf
__global__ void pv_sqrt_sweep_kernel(uint32_t first, uint64_t count, unsigned long long *res) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long bad = 0;
    uint32_t first_bad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
        const uint32_t u = first + (uint32_t)i;
        const float a = pv_u2f(u);
        if (pv_f2u(pv_sqrt_safe(a)) != pv_f2u(sqrtf(a))) {
            if (!bad) first_bad = u;
            ++bad;
        }
    }
    if (bad) {
        atomicAdd(&res[0], bad);
        atomicMin(&res[1], (unsigned long long)first_bad);
    }
}

constexpr int kSlots = 3; // groups in flight

} // namespace

struct pv_hostio {
    pv_batch *batch = nullptr;
    int device = 0, channels = 0, wire = 0;
    int32_t nstreams = 0, per_group = 0;
    int64_t frames = 0, out_frames = 0;
    float *d_in[kSlots] = {}, *d_out[kSlots] = {};
    int16_t *d_in16[kSlots] = {}, *d_out16[kSlots] = {};
    hipStream_t s_up = nullptr, s_run = nullptr, s_down = nullptr;
    hipEvent_t ev_up[kSlots] = {}, ev_run[kSlots] = {}, ev_down[kSlots] = {};
    int64_t staging_bytes = 0;
    // segmented object (pv_hostio_create_segmented): per_group == nstreams, the slots hold row windows of `pitch` samples
    bool segmented = false;
    int64_t pitch_in = 0, pitch_out = 0;
    std::vector<pv_batch_span_info> segs;
};

extern "C" {

int pv_debug_atan2f(const float *y, const float *x, float *out, int64_t n, int device) {
    if (n < 0 || (n > 0 && (!y || !x || !out))) return PV_ERR_INVALID_ARG;
    if (n == 0) return PV_OK;
    float *d = nullptr;
    if (hipSetDevice(device) != hipSuccess || hipMalloc((void **)&d, (size_t)n * 3 * sizeof(float)) != hipSuccess)
        return PV_ERR_HIP;
    bool ok = hipMemcpy(d, y, (size_t)n * 4, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(d + n, x, (size_t)n * 4, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(pv_atan2f_probe, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, d, d + n, d + 2 * n, n);
        ok = hipMemcpy(out, d + 2 * n, (size_t)n * 4, hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(d);
    return ok ? PV_OK : PV_ERR_HIP;
}

int pv_debug_polar(const float *im, const float *re, float *phase, float *mag, int64_t n, int device) {
    if (n < 0 || (n > 0 && (!im || !re || !phase || !mag))) return PV_ERR_INVALID_ARG;
    if (n == 0) return PV_OK;
    float *d = nullptr;
    if (hipSetDevice(device) != hipSuccess || hipMalloc((void **)&d, (size_t)n * 4 * sizeof(float)) != hipSuccess)
        return PV_ERR_HIP;
    bool ok = hipMemcpy(d, im, (size_t)n * 4, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(d + n, re, (size_t)n * 4, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(pv_polar_probe, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, d, d + n, d + 2 * n,
                           d + 3 * n, n);
        ok = hipMemcpy(phase, d + 2 * n, (size_t)n * 4, hipMemcpyDeviceToHost) == hipSuccess &&
             hipMemcpy(mag, d + 3 * n, (size_t)n * 4, hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(d);
    return ok ? PV_OK : PV_ERR_HIP;
}

int pv_debug_sqrt_sweep(uint32_t first_bits, uint64_t count, uint64_t *mismatches, uint32_t *first_bad, int device) {
    if (!mismatches || !first_bad) return PV_ERR_INVALID_ARG;
    unsigned long long *d = nullptr, h[2] = {0ull, ~0ull};
    if (hipSetDevice(device) != hipSuccess || hipMalloc((void **)&d, sizeof(h)) != hipSuccess) return PV_ERR_HIP;
    bool ok = hipMemcpy(d, h, sizeof(h), hipMemcpyHostToDevice) == hipSuccess;
    if (ok && count) {
        hipLaunchKernelGGL(pv_sqrt_sweep_kernel, dim3(4096), dim3(256), 0, nullptr, first_bits, (uint64_t)count, d);
        ok = hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(d);
    *mismatches = h[0];
    *first_bad = (uint32_t)h[1];
    return ok ? PV_OK : PV_ERR_HIP;
}

void *pv_host_alloc(size_t bytes) {
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}
void pv_host_free(void *p) {
    if (p) (void)hipHostFree(p);
}

void pv_hostio_destroy(pv_hostio *h) {
    if (!h) return;
    for (int i = 0; i < kSlots; ++i) {
        if (h->d_in[i]) (void)hipFree(h->d_in[i]);
        if (h->d_out[i]) (void)hipFree(h->d_out[i]);
        if (h->d_in16[i]) (void)hipFree(h->d_in16[i]);
        if (h->d_out16[i]) (void)hipFree(h->d_out16[i]);
        if (h->ev_up[i]) (void)hipEventDestroy(h->ev_up[i]);
        if (h->ev_run[i]) (void)hipEventDestroy(h->ev_run[i]);
        if (h->ev_down[i]) (void)hipEventDestroy(h->ev_down[i]);
    }
    if (h->s_up) (void)hipStreamDestroy(h->s_up);
    if (h->s_run) (void)hipStreamDestroy(h->s_run);
    if (h->s_down) (void)hipStreamDestroy(h->s_down);
    pv_batch_destroy(h->batch);
    delete h;
}

int64_t pv_hostio_out_frames(const pv_hostio *h) { return h ? h->out_frames : -1; }

#define HIO(call)                         \
    do {                                  \
        if ((call) != hipSuccess) {       \
            pv_hostio_destroy(h);         \
            return PV_ERR_HIP;            \
        }                                 \
    } while (0)

int pv_hostio_create(const pv_config *cfg, int32_t nstreams, int64_t frames, int32_t block, int32_t flush, int device,
                     int32_t streams_per_group, int32_t wire, pv_hostio **out) {
    if (!cfg || !out || nstreams < 1 || frames < 1 || streams_per_group < 1 || (wire != PV_WIRE_F32 && wire != PV_WIRE_I16))
        return PV_ERR_INVALID_ARG;
    *out = nullptr;
    pv_hostio *h = new pv_hostio();
    h->device = device;
    h->channels = cfg->channels;
    h->wire = wire;
    h->nstreams = nstreams;
    h->per_group = streams_per_group < nstreams ? streams_per_group : nstreams;
    h->frames = frames;
    // one batch engine of a group's size serves every group in turn (the last group may be smaller: it runs as a
    // full group whose surplus streams read and write the slot's own buffer and are not copied back)
    int st = pv_batch_create(cfg, h->per_group, frames, block, flush, device, &h->batch);
    if (st != PV_OK) {
        delete h;
        return st;
    }
    h->out_frames = pv_batch_out_frames(h->batch);
    const size_t n_in = (size_t)h->per_group * h->channels * (size_t)frames;
    const size_t n_out = (size_t)h->per_group * h->channels * (size_t)(h->out_frames > 0 ? h->out_frames : 1);
    HIO(hipSetDevice(device));
    h->staging_bytes = (int64_t)kSlots * (int64_t)(n_in + n_out) *
                       (int64_t)(sizeof(float) + (wire == PV_WIRE_I16 ? sizeof(int16_t) : 0));
    for (int i = 0; i < kSlots; ++i) {
        HIO(hipMalloc((void **)&h->d_in[i], n_in * sizeof(float)));
        HIO(hipMemset(h->d_in[i], 0, n_in * sizeof(float)));
        HIO(hipMalloc((void **)&h->d_out[i], n_out * sizeof(float)));
        if (wire == PV_WIRE_I16) {
            HIO(hipMalloc((void **)&h->d_in16[i], n_in * sizeof(int16_t)));
            HIO(hipMalloc((void **)&h->d_out16[i], n_out * sizeof(int16_t)));
        }
        HIO(hipEventCreateWithFlags(&h->ev_up[i], hipEventDisableTiming));
        HIO(hipEventCreateWithFlags(&h->ev_run[i], hipEventDisableTiming));
        HIO(hipEventCreateWithFlags(&h->ev_down[i], hipEventDisableTiming));
    }
    HIO(hipStreamCreateWithFlags(&h->s_up, hipStreamNonBlocking));
    HIO(hipStreamCreateWithFlags(&h->s_run, hipStreamNonBlocking));
    HIO(hipStreamCreateWithFlags(&h->s_down, hipStreamNonBlocking));
    *out = h;
    return PV_OK;
}

int pv_hostio_create_segmented(const pv_config *cfg, int32_t nstreams, int64_t frames, int32_t block, int32_t flush,
                               int device, int32_t launches_per_segment, int32_t wire, pv_hostio **out) {
    if (!cfg || !out || nstreams < 1 || frames < 1 || launches_per_segment < 1 ||
        (wire != PV_WIRE_F32 && wire != PV_WIRE_I16))
        return PV_ERR_INVALID_ARG;
    *out = nullptr;
    pv_hostio *h = new pv_hostio();
    h->device = device;
    h->channels = cfg->channels;
    h->wire = wire;
    h->nstreams = nstreams;
    h->per_group = nstreams;
    h->frames = frames;
    h->segmented = true;
    // ONE batch of every stream; a segment is a span of its launches
    int st = pv_batch_create(cfg, nstreams, frames, block, flush, device, &h->batch);
    if (st != PV_OK) {
        delete h;
        return st;
    }
    h->out_frames = pv_batch_out_frames(h->batch);
    const int32_t L = pv_batch_launches(h->batch);
    // the windows are sized for any span of that many launches (pv_plan.cc batch_span_bounds), not for this job's
    // spans: the staging memory is the same whatever `frames` is
    int64_t max_in = 0, max_out = 0;
    {
        pv::Derived d;
        if ((st = pv::derive(*cfg, d)) != PV_OK) {
            pv_hostio_destroy(h);
            return st;
        }
        // (the batch above was created under this setting and environment a moment ago)
        const int Tc = pv::batch_chunk_slices(*cfg, nstreams, pv_get_arithmetic() == PV_ARITH_FAST);
        pv::batch_span_bounds(d, Tc, launches_per_segment, max_in, max_out);
    }
    for (int32_t f = 0; f < L; f += launches_per_segment) {
        pv_batch_span_info sp;
        st = pv_batch_span(h->batch, f, L - f < launches_per_segment ? L - f : launches_per_segment, &sp);
        if (st == PV_OK && (sp.in_end - sp.in_begin > max_in || sp.out_end - sp.out_begin > max_out)) st = PV_ERR_UNSUPPORTED;
        if (st != PV_OK) {
            pv_hostio_destroy(h);
            return st;
        }
        h->segs.push_back(sp);
    }
    // window pitches in samples: multiples of 8, so that rows of float AND of int16 start on 16-byte boundaries
    h->pitch_in = ((max_in > 0 ? max_in : 1) + 7) & ~(int64_t)7;
    h->pitch_out = ((max_out > 0 ? max_out : 1) + 7) & ~(int64_t)7;
    const size_t rows = (size_t)nstreams * (size_t)h->channels;
    const size_t n_in = rows * (size_t)h->pitch_in, n_out = rows * (size_t)h->pitch_out;
    // (the conversion kernels' one-dimensional grids: rows x ceil(pitch / 2048) workgroups)
    if (rows * (size_t)((h->pitch_in > h->pitch_out ? h->pitch_in : h->pitch_out) / 2048 + 1) > 0x7fffffffull) {
        pv_hostio_destroy(h);
        return PV_ERR_UNSUPPORTED;
    }
    h->staging_bytes = (int64_t)kSlots * (int64_t)(n_in + n_out) *
                       (int64_t)(sizeof(float) + (wire == PV_WIRE_I16 ? sizeof(int16_t) : 0));
    HIO(hipSetDevice(device));
    for (int i = 0; i < kSlots; ++i) {
        HIO(hipMalloc((void **)&h->d_in[i], n_in * sizeof(float)));
        HIO(hipMemset(h->d_in[i], 0, n_in * sizeof(float)));
        HIO(hipMalloc((void **)&h->d_out[i], n_out * sizeof(float)));
        if (wire == PV_WIRE_I16) {
            HIO(hipMalloc((void **)&h->d_in16[i], n_in * sizeof(int16_t)));
            HIO(hipMalloc((void **)&h->d_out16[i], n_out * sizeof(int16_t)));
        }
        HIO(hipEventCreateWithFlags(&h->ev_up[i], hipEventDisableTiming));
        HIO(hipEventCreateWithFlags(&h->ev_run[i], hipEventDisableTiming));
        HIO(hipEventCreateWithFlags(&h->ev_down[i], hipEventDisableTiming));
    }
    HIO(hipStreamCreateWithFlags(&h->s_up, hipStreamNonBlocking));
    HIO(hipStreamCreateWithFlags(&h->s_run, hipStreamNonBlocking));
    HIO(hipStreamCreateWithFlags(&h->s_down, hipStreamNonBlocking));
    *out = h;
    return PV_OK;
}
#undef HIO

int64_t pv_hostio_staging_bytes(const pv_hostio *h) { return h ? h->staging_bytes : -1; }

// One segment after the other through the three window slots: rows' [in_begin, in_end) up (pitched copy), the span,
// rows' [out_begin, out_end) down; events chain the three streams exactly as the grouped loop below does.
static int hostio_run_segmented(pv_hostio *h, const void *host_in, void *host_out) {
    const bool i16 = h->wire == PV_WIRE_I16;
    const size_t esz = i16 ? sizeof(int16_t) : sizeof(float);
    const int rows = h->nstreams * h->channels;
    for (size_t g = 0; g < h->segs.size(); ++g) {
        const pv_batch_span_info &sp = h->segs[g];
        const int slot = (int)(g % kSlots);
        const int64_t in_len = sp.in_end - sp.in_begin, out_len = sp.out_end - sp.out_begin;
        // up: the slot's input window is free once the span that read it (three segments ago) has finished
        if (g >= (size_t)kSlots && hipStreamWaitEvent(h->s_up, h->ev_run[slot], 0) != hipSuccess) return PV_ERR_HIP;
        void *d_up = i16 ? (void *)h->d_in16[slot] : (void *)h->d_in[slot];
        if (in_len > 0 && hipMemcpy2DAsync(d_up, (size_t)h->pitch_in * esz, (const char *)host_in + (size_t)sp.in_begin * esz,
                                           (size_t)h->frames * esz, (size_t)in_len * esz, (size_t)rows,
                                           hipMemcpyHostToDevice, h->s_up) != hipSuccess)
            return PV_ERR_HIP;
        if (hipEventRecord(h->ev_up[slot], h->s_up) != hipSuccess) return PV_ERR_HIP;
        // run: after the input has arrived and the slot's output window has left (three segments ago)
        if (hipStreamWaitEvent(h->s_run, h->ev_up[slot], 0) != hipSuccess) return PV_ERR_HIP;
        if (g >= (size_t)kSlots && hipStreamWaitEvent(h->s_run, h->ev_down[slot], 0) != hipSuccess) return PV_ERR_HIP;
        if (i16 && in_len > 0)
            hipLaunchKernelGGL(pv_rows_i16_to_f32, dim3((unsigned)rows * (unsigned)((in_len + 2047) / 2048)), dim3(256), 0,
                               h->s_run, h->d_in16[slot], h->d_in[slot], rows, in_len, h->pitch_in,
                               (unsigned)((in_len + 2047) / 2048));
        const int st = pv_batch_run_span(h->batch, sp.first_launch, sp.launches, h->d_in[slot], h->pitch_in, h->d_out[slot],
                                         h->pitch_out, (void *)h->s_run);
        if (st != PV_OK) return st;
        if (i16 && out_len > 0)
            hipLaunchKernelGGL(pv_rows_f32_to_i16, dim3((unsigned)rows * (unsigned)((out_len + 2047) / 2048)), dim3(256), 0,
                               h->s_run, h->d_out[slot], h->d_out16[slot], rows, out_len, h->pitch_out,
                               (unsigned)((out_len + 2047) / 2048));
        if (hipEventRecord(h->ev_run[slot], h->s_run) != hipSuccess) return PV_ERR_HIP;
        // down
        if (hipStreamWaitEvent(h->s_down, h->ev_run[slot], 0) != hipSuccess) return PV_ERR_HIP;
        const void *d_dn = i16 ? (const void *)h->d_out16[slot] : (const void *)h->d_out[slot];
        if (out_len > 0 && hipMemcpy2DAsync((char *)host_out + (size_t)sp.out_begin * esz, (size_t)h->out_frames * esz, d_dn,
                                            (size_t)h->pitch_out * esz, (size_t)out_len * esz, (size_t)rows,
                                            hipMemcpyDeviceToHost, h->s_down) != hipSuccess)
            return PV_ERR_HIP;
        if (hipEventRecord(h->ev_down[slot], h->s_down) != hipSuccess) return PV_ERR_HIP;
    }
    if (hipStreamSynchronize(h->s_down) != hipSuccess || hipStreamSynchronize(h->s_run) != hipSuccess ||
        hipStreamSynchronize(h->s_up) != hipSuccess)
        return PV_ERR_HIP;
    return hipGetLastError() == hipSuccess ? PV_OK : PV_ERR_HIP;
}

int pv_hostio_run(pv_hostio *h, const void *host_in, void *host_out) {
    if (!h || !host_in || (!host_out && h->out_frames > 0)) return PV_ERR_INVALID_ARG;
    if (hipSetDevice(h->device) != hipSuccess) return PV_ERR_HIP;
    if (h->segmented) return hostio_run_segmented(h, host_in, host_out);
    const size_t esz = h->wire == PV_WIRE_I16 ? sizeof(int16_t) : sizeof(float);
    const size_t row_in = (size_t)h->channels * (size_t)h->frames, row_out = (size_t)h->channels * (size_t)h->out_frames;
    const int groups = (h->nstreams + h->per_group - 1) / h->per_group;
    for (int g = 0; g < groups; ++g) {
        const int slot = g % kSlots;
        const int s0 = g * h->per_group;
        const int ns = h->nstreams - s0 < h->per_group ? h->nstreams - s0 : h->per_group;
        const size_t n_in = (size_t)ns * row_in, n_out = (size_t)ns * row_out;
        // up: the slot's input buffer is free once the run that read it (three groups ago) has finished
        if (g >= kSlots && hipStreamWaitEvent(h->s_up, h->ev_run[slot], 0) != hipSuccess) return PV_ERR_HIP;
        void *d_up = h->wire == PV_WIRE_I16 ? (void *)h->d_in16[slot] : (void *)h->d_in[slot];
        if (hipMemcpyAsync(d_up, (const char *)host_in + (size_t)s0 * row_in * esz, n_in * esz, hipMemcpyHostToDevice,
                           h->s_up) != hipSuccess)
            return PV_ERR_HIP;
        if (hipEventRecord(h->ev_up[slot], h->s_up) != hipSuccess) return PV_ERR_HIP;
        // run: after the input has arrived and the slot's output buffer has left (three groups ago)
        if (hipStreamWaitEvent(h->s_run, h->ev_up[slot], 0) != hipSuccess) return PV_ERR_HIP;
        if (g >= kSlots && hipStreamWaitEvent(h->s_run, h->ev_down[slot], 0) != hipSuccess) return PV_ERR_HIP;
        if (h->wire == PV_WIRE_I16)
            hipLaunchKernelGGL(pv_i16_to_f32, dim3((unsigned)((n_in + 255) / 256)), dim3(256), 0, h->s_run,
                               h->d_in16[slot], h->d_in[slot], (int64_t)n_in);
        const int st = pv_batch_run(h->batch, h->d_in[slot], h->d_out[slot], (void *)h->s_run);
        if (st != PV_OK) return st;
        if (h->wire == PV_WIRE_I16 && n_out > 0)
            hipLaunchKernelGGL(pv_f32_to_i16, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, h->s_run,
                               h->d_out[slot], h->d_out16[slot], (int64_t)n_out);
        if (hipEventRecord(h->ev_run[slot], h->s_run) != hipSuccess) return PV_ERR_HIP;
        // down
        if (hipStreamWaitEvent(h->s_down, h->ev_run[slot], 0) != hipSuccess) return PV_ERR_HIP;
        const void *d_dn = h->wire == PV_WIRE_I16 ? (const void *)h->d_out16[slot] : (const void *)h->d_out[slot];
        if (n_out > 0 && hipMemcpyAsync((char *)host_out + (size_t)s0 * row_out * esz, d_dn, n_out * esz,
                                        hipMemcpyDeviceToHost, h->s_down) != hipSuccess)
            return PV_ERR_HIP;
        if (hipEventRecord(h->ev_down[slot], h->s_down) != hipSuccess) return PV_ERR_HIP;
    }
    if (hipStreamSynchronize(h->s_down) != hipSuccess || hipStreamSynchronize(h->s_run) != hipSuccess ||
        hipStreamSynchronize(h->s_up) != hipSuccess)
        return PV_ERR_HIP;
    return hipGetLastError() == hipSuccess ? PV_OK : PV_ERR_HIP;
}

} // extern "C"
