// pv_snapshot.h -- the blob of a stream-pool slot (include/audiomod_pv.h "Stream pool snapshots"): its header, the
// encoding of the slot's host state, the checksum and the validator.  Pure host C++ over pv_plan.h's types: no HIP, so
// that tests/native/host_snapshot.cc drives it with plain g++.  pv_engine.cc (pv_pool_save / pv_pool_restore /
// pv_pool_blob_info) uses these functions and does not restate them.
//
// Layout, little-endian, no pointers, every part at a multiple of 16 bytes from the blob's start:
//   Header                         fixed size: magic, version, total length, the stream's configuration, the geometry
//                                  of the pool that wrote it, counters, Planner::State, the sizes of what follows
//   nlive  x LiveFrame             the overlap-add builder's live frames, oldest first
//   C x pending floats             output made but not yet retrieved, channel after channel
//   nseg   x SegEntry              directory of the device payload: which per-row buffer, how many bytes
//   payload                        the slot's rows of each buffer of the directory, in its order, each padded to 16 bytes
//   uint64 checksum                hash64 of everything before it
// A blob is NOT a trust boundary: the payload holds peak counts, step modes and ring positions that kernels use as
// indices.  validate() guards against truncation and accidental corruption (length, magic, version, every internal size
// against the header's geometry, then the checksum); it cannot tell a forged blob from a real one.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

#include "pv_plan.h"
#include "pv_whisper.h"

namespace pv {
namespace snap {

static_assert(__BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__, "the blob format is little-endian and written from memory");

constexpr uint64_t kMagic = 0x4e534c4f4f505650ull; // "PVPOOLSN"
constexpr uint32_t kVersion = 1;
// A slot with the WHISPER voice (include/audiomod_pv.h "Voice setting"): the header's mode reads PV_MODE_WHISPER -- the
// stream is that engine's -- and the directory ends with the slot's generator state row (pv_whisper.h).  Only such blobs
// carry this version: a robotic slot's blob is version 1, byte for byte what it always was.
constexpr uint32_t kVersionVoice = 2;
// A slot with a carrier (include/audiomod_pv.h "Carrier setting"): the header's mode reads PV_MODE_VOCODER_ROSENBERG or
// PV_MODE_VOCODER_CHORD -- the stream is that engine's, and so are the planner state and the live frames.  The payload
// is a robotic slot's: the slot's row of the carrier ring is NOT saved.  The carrier is a closed form of the sample
// position, so pv_pool_restore leaves the row to the slot's next launch group, which rewrites everything its frames
// read (from the group's first frame on); the carrier planes hold nothing that outlives a launch.  Two saves of one
// stream history are therefore byte-identical whatever the rows held.
constexpr uint32_t kVersionCarrier = 3;
inline uint32_t version_of(int32_t mode) {
    return mode == PV_MODE_WHISPER ? kVersionVoice
           : (mode == PV_MODE_VOCODER_ROSENBERG || mode == PV_MODE_VOCODER_CHORD) ? kVersionCarrier
                                                                                   : kVersion;
}

// The per-row device buffers a slot carries between calls, in payload order.  Which of them a configuration has follows
// from its phase stage and from whether its pool keeps an overlap-add stream ring (seg_bytes).
enum Buf : int32_t {
    kBufIn = 0,   // input ring                  [C][ring] float
    kBufMag,      // magnitude planes            [C][TR][HP] float
    kBufPhase,    // analysis phase planes       [C][TR][HP] float
    kBufOutphase, // output phase planes         [C][TR][HP] float
    kBufPeaks,    // peak lists                  [C][TR][PKP] uint16
    kBufNpk,      // peak counts                 [C][TR] int32
    kBufRecs,     // peak records                [C][TR][PKP] 16 bytes
    kBufModes,    // step modes                  [C][TR] int32
    kBufRot,      // rotations                   [C][TR][PKP] float
    kBufStPp,     // previous analysis phase     [C][hs] float
    kBufStPo,     // previous output phase       [C][hs] float
    kBufStRot,    // previous rotations          [C][PKP] float
    kBufStKind,   // kind of the carried state   [C] int32
    kBufAcc,      // accumulator images          [2][C][AR] float
    kBufStream,   // overlap-add stream ring     [C][stream_len] float
    kBufWhisper,  // generator state row         [kWhisperStatePitch] uint32 (version 2 blobs)
    kBufCount
};

struct Header {
    uint64_t magic;
    uint32_t version, header_bytes;
    uint64_t total_bytes;
    // the stream: its pool's configuration with the slot's own time ratio and pitch
    int32_t sample_rate, channels;
    float time_ratio, pitch_semitones;
    int32_t mode, coremode, fftsize, hopsize;
    int32_t arith;       // PV_ARITH_* the pool was created under
    int32_t phase_stage; // -1 none, 0 propagation, 1 match + rotation chain, 2 none (synthesis reads the analysis phases)
    // geometry of the pool's per-row buffers
    int32_t N, hs, ring, TR, HP, PKP, AR, stream_len; // stream_len 0: the pool keeps no stream ring
    // host state
    int64_t fed, uploaded, slices;
    int64_t pl_in_fill, pl_out_fill, pl_slices, pl_dropped, pl_K, pl_P, pl_prev_increment; // Planner::State
    float pl_recovery, pl_divergence;
    int32_t acc_half, any_upper_skip;
    int32_t nlive, nseg;
    int64_t pending;                   // frames of output not yet retrieved
    int64_t host_bytes, payload_bytes; // live frames + pending output (padded); directory + payload
};
static_assert(sizeof(Header) == 224, "Header has no implicit padding");

struct LiveFrame { // ChainBuilder::Live
    int64_t P;
    int32_t flags, pad;
};
static_assert(sizeof(LiveFrame) == 16, "");
struct SegEntry {
    int32_t buf, pad;
    int64_t bytes; // unpadded
};
static_assert(sizeof(SegEntry) == 16, "");

// everything of a slot that lives on the host
struct HostState {
    Planner::State plan{};
    int64_t fed = 0, uploaded = 0, slices = 0;
    int32_t acc_half = 0;
    bool any_upper_skip = false;
    std::vector<LiveFrame> live;
};

inline int64_t pad16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// bytes of a slot's rows of `buf` under h's geometry; 0 for a buffer the configuration does not have
inline int64_t seg_bytes(const Header &h, int buf) {
    const int64_t C = h.channels, planes = C * h.TR;
    const bool chain = h.phase_stage == 1, carried = h.phase_stage == 0 || h.phase_stage == 1;
    switch (buf) {
    case kBufIn: return C * h.ring * 4;
    case kBufMag: case kBufPhase: return planes * h.HP * 4;
    case kBufOutphase: return carried ? planes * h.HP * 4 : 0;
    case kBufPeaks: return chain ? planes * h.PKP * 2 : 0;
    case kBufNpk: case kBufModes: return chain ? planes * 4 : 0;
    case kBufRecs: return chain ? planes * h.PKP * 16 : 0;
    case kBufRot: return chain ? planes * h.PKP * 4 : 0;
    case kBufStPp: case kBufStPo: return carried ? C * h.hs * 4 : 0;
    case kBufStRot: return chain ? C * h.PKP * 4 : 0;
    case kBufStKind: return chain ? C * 4 : 0;
    case kBufAcc: return 2 * C * h.AR * 4;
    case kBufStream: return C * (int64_t)h.stream_len * 4;
    case kBufWhisper: return h.mode == PV_MODE_WHISPER ? (int64_t)kWhisperStatePitch * 4 : 0;
    default: return 0;
    }
}

// Any simple 64-bit hash: eight bytes at a time, each step a bijection of the running value for a given word and
// injective in the word for a given running value, so a change confined to one word always changes the result.
inline uint64_t hash64(const uint8_t *p, size_t n) {
    uint64_t h = 0x9e3779b97f4a7c15ull ^ (uint64_t)n;
    size_t i = 0;
    for (; i + 8 <= n; i += 8) {
        uint64_t w;
        memcpy(&w, p + i, 8);
        h = (h ^ w) * 0x100000001b3ull;
        h ^= h >> 32;
    }
    if (i < n) {
        uint64_t w = 0;
        memcpy(&w, p + i, n - i);
        h = (h ^ w) * 0x100000001b3ull;
        h ^= h >> 32;
    }
    return h;
}

// Fills the sizes of h (nlive, pending, nseg, host_bytes, payload_bytes, total_bytes, magic, version) from its
// configuration and geometry fields, which the caller has set.
inline void fill_sizes(Header &h, int32_t nlive, int64_t pending) {
    h.magic = kMagic;
    h.version = version_of(h.mode);
    h.header_bytes = (uint32_t)sizeof(Header);
    h.nlive = nlive;
    h.pending = pending;
    h.host_bytes = (int64_t)nlive * (int64_t)sizeof(LiveFrame) + pad16((int64_t)h.channels * pending * 4);
    h.nseg = 0;
    int64_t pay = 0;
    for (int b = 0; b < kBufCount; ++b)
        if (const int64_t n = seg_bytes(h, b)) {
            ++h.nseg;
            pay += pad16(n);
        }
    h.payload_bytes = (int64_t)h.nseg * (int64_t)sizeof(SegEntry) + pay;
    h.total_bytes = (uint64_t)((int64_t)sizeof(Header) + h.host_bytes + h.payload_bytes + 8);
}

inline int64_t host_offset(const Header &) { return (int64_t)sizeof(Header); }
inline int64_t dir_offset(const Header &h) { return (int64_t)sizeof(Header) + h.host_bytes; }
// where the rows of the first buffer of the directory start; the others follow, each padded to 16 bytes
inline int64_t payload_offset(const Header &h) { return dir_offset(h) + (int64_t)h.nseg * (int64_t)sizeof(SegEntry); }
inline int64_t device_bytes(const Header &h) { return h.payload_bytes - (int64_t)h.nseg * (int64_t)sizeof(SegEntry); }

inline void state_to_header(const HostState &s, Header &h) {
    h.fed = s.fed, h.uploaded = s.uploaded, h.slices = s.slices;
    h.pl_in_fill = s.plan.in_fill, h.pl_out_fill = s.plan.out_fill, h.pl_slices = s.plan.slices;
    h.pl_dropped = s.plan.dropped, h.pl_K = s.plan.K, h.pl_P = s.plan.P, h.pl_prev_increment = s.plan.prev_increment;
    h.pl_recovery = s.plan.recovery, h.pl_divergence = s.plan.divergence;
    h.acc_half = s.acc_half;
    h.any_upper_skip = s.any_upper_skip ? 1 : 0;
}

// Writes everything but the device payload and the checksum: the header (state and sizes filled in here from `s` and
// `pending`), the live frames, the pending output (pending_ch[c]: `pending` floats of channel c) and the directory.
// `blob` has h.total_bytes bytes.  The caller then copies the device rows to payload_offset() on and calls seal().
inline void encode_head(Header &h, const HostState &s, const float *const *pending_ch, int64_t pending, uint8_t *blob) {
    state_to_header(s, h);
    fill_sizes(h, (int32_t)s.live.size(), pending);
    memcpy(blob, &h, sizeof h);
    uint8_t *q = blob + host_offset(h);
    memset(q, 0, (size_t)h.host_bytes);
    for (const LiveFrame &f : s.live) {
        const LiveFrame g{f.P, f.flags, 0};
        memcpy(q, &g, sizeof g);
        q += sizeof g;
    }
    for (int c = 0; c < h.channels && pending > 0; ++c) memcpy(q + (size_t)c * pending * 4, pending_ch[c], (size_t)pending * 4);
    q = blob + dir_offset(h);
    for (int b = 0; b < kBufCount; ++b)
        if (const int64_t n = seg_bytes(h, b)) {
            const SegEntry e{b, 0, n};
            memcpy(q, &e, sizeof e);
            q += sizeof e;
        }
}

inline void seal(uint8_t *blob, const Header &h) {
    const uint64_t sum = hash64(blob, (size_t)h.total_bytes - 8);
    memcpy(blob + h.total_bytes - 8, &sum, 8);
}

// Validates `bytes` bytes at `blob`, in this order: length, magic, version, every internal size against the header's
// geometry, the checksum.  Reads nothing beyond `bytes`.  Returns nullptr and the header in *out for a valid blob, else
// why not (static text).
inline const char *validate(const void *blob, int64_t bytes, Header *out) {
    if (!blob) return "no blob";
    if (bytes < (int64_t)sizeof(Header) + 8) return "shorter than a header";
    const uint8_t *p = static_cast<const uint8_t *>(blob);
    Header h;
    memcpy(&h, p, sizeof h);
    if (h.total_bytes != (uint64_t)bytes) return "its length differs from the one its header states (truncated?)";
    if (h.magic != kMagic) return "not a stream-pool snapshot (magic)";
    if (h.version != kVersion && h.version != kVersionVoice && h.version != kVersionCarrier) return "an unknown format version";
    if (h.version != version_of(h.mode)) return "its format version does not go with its mode";
    if (h.header_bytes != sizeof(Header)) return "header size";
    auto in = [](int64_t v, int64_t lo, int64_t hi) { return v >= lo && v <= hi; };
    if (!in(h.channels, 1, 65535) || !in(h.N, 2, 1 << 16) || h.hs != h.N / 2 || !in(h.ring, 1, 1 << 28) ||
        (h.ring & (h.ring - 1)) || !in(h.TR, 2, 1 << 12) || !in(h.HP, h.hs, 1 << 17) || !in(h.PKP, 1, 1 << 16) ||
        !in(h.AR, h.N, 1 << 17) || !in(h.stream_len, 0, 1 << 28) || (h.stream_len & (h.stream_len - 1)) ||
        !in(h.phase_stage, -1, 2) || !in(h.arith, 0, 1) || !in(h.acc_half, 0, 1) || !in(h.any_upper_skip, 0, 1))
        return "a geometry field out of range";
    if (!in(h.nlive, 0, 1 << 20) || !in(h.pending, 0, (int64_t)1 << 31) || h.fed < 0 || h.uploaded < 0 ||
        h.uploaded > h.fed || h.slices < 0 || h.pl_slices < 0 || h.pl_out_fill < 0)
        return "a counter out of range";
    Header want = h;
    fill_sizes(want, h.nlive, h.pending);
    if (want.nseg != h.nseg || want.host_bytes != h.host_bytes || want.payload_bytes != h.payload_bytes ||
        want.total_bytes != h.total_bytes)
        return "its sizes do not follow from its geometry";
    const uint8_t *q = p + dir_offset(h);
    for (int b = 0; b < kBufCount; ++b)
        if (const int64_t n = seg_bytes(h, b)) {
            SegEntry e;
            memcpy(&e, q, sizeof e);
            q += sizeof e;
            if (e.buf != b || e.bytes != n) return "its directory does not follow from its geometry";
        }
    uint64_t sum;
    memcpy(&sum, p + bytes - 8, 8);
    if (sum != hash64(p, (size_t)bytes - 8)) return "checksum mismatch (corrupted)";
    if (out) *out = h;
    return nullptr;
}

// the host state of a VALIDATED blob
inline void decode_host(const void *blob, const Header &h, HostState &s) {
    s.fed = h.fed, s.uploaded = h.uploaded, s.slices = h.slices;
    s.plan = Planner::State{h.pl_in_fill, h.pl_out_fill, h.pl_slices, h.pl_dropped, h.pl_K, h.pl_P, h.pl_prev_increment,
                            h.pl_recovery, h.pl_divergence};
    s.acc_half = h.acc_half;
    s.any_upper_skip = h.any_upper_skip != 0;
    s.live.resize((size_t)h.nlive);
    if (h.nlive) memcpy(s.live.data(), static_cast<const uint8_t *>(blob) + host_offset(h), (size_t)h.nlive * sizeof(LiveFrame));
}
// ... and its pending output: `pending` floats of channel c (unaligned: copy, do not dereference)
inline const uint8_t *pending_of(const void *blob, const Header &h, int c) {
    return static_cast<const uint8_t *>(blob) + host_offset(h) + (int64_t)h.nlive * (int64_t)sizeof(LiveFrame) +
           (int64_t)c * h.pending * 4;
}

} // namespace snap
} // namespace pv
