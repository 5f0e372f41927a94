// plane_check.h -- the layout rules of the C ABI (include/fiunet.h), each in one place: what stands between a caller's
// numbers and a kernel's addresses.  Host only: integer arithmetic on the ABI's own structs, no HIP and
// no state, so a plain host compiler builds it alone (tests/host_checks/plane_check_main.cpp).  A check returns the reason
// of its refusal or nullptr, and the entry point turns the reason into fail(code, reason).  Every product is guarded by a
// division or a bound before it is formed: no unsigned arithmetic here wraps, on any input.
#pragma once
#include "../../include/fiunet.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace fiunet {

// ---- fiunet_resize_plane: sample (y, x) of frame f lies at offset + f * frame_stride + y * pitch + x * step ----
// The rule of one plane: sides 1..max_side (at most 2^24), step 1..4, a pitch that covers a row, frame 0 inside the frame
// stride.  `filter` is not looked at: its rule differs between source planes, destination planes and warps.
inline const char* plane_check(const fiunet_resize_plane& p, int max_side)
{
    if (p.h < 1 || p.w < 1) return "a plane's h and w must be positive";
    if (p.h > max_side || p.w > max_side)
        return max_side == 32768 ? "a plane's h and w must not exceed 32768" : "a plane's h and w must not exceed 2^24";
    if (p.step < 1 || p.step > 4) return "a plane's step must be 1..4";
    const size_t row = (size_t)(p.w - 1) * (size_t)p.step + 1;   // (below 2^26)
    if (p.pitch < row) return "a plane's pitch must cover a row: (w - 1) * step + 1";
    if (p.h > 1 && p.pitch > (SIZE_MAX - row) / (size_t)(p.h - 1)) return "a plane's pitch is too large";
    const size_t body = (size_t)(p.h - 1) * p.pitch + row;
    if (p.offset > p.frame_stride || body > p.frame_stride - p.offset) return "a plane must lie inside its frame stride";
    return nullptr;
}

// samples from the first sample of a frame of a checked plane to behind its last
inline size_t plane_body(const fiunet_resize_plane& p) { return (size_t)(p.h - 1) * p.pitch + (size_t)(p.w - 1) * (size_t)p.step + 1; }

// The bytes [lo, hi) that n >= 1 frames of a checked plane cover in a buffer of `sample_bytes`-byte samples at `base`;
// false where they leave the address space (n frame strides, as bytes, must fit behind the plane's first frame).
inline bool plane_range(const void* base, size_t sample_bytes, const fiunet_resize_plane& p, int n, uintptr_t* lo, uintptr_t* hi)
{
    const size_t body = plane_body(p), room = SIZE_MAX / sample_bytes;   // (offset + body <= frame_stride: plane_check)
    if (p.offset + body > room || p.frame_stride > (room - body - p.offset) / (size_t)n) return false;
    const size_t end = (p.offset + (size_t)(n - 1) * p.frame_stride + body) * sample_bytes;
    if (end > UINTPTR_MAX - (uintptr_t)base) return false;
    *lo = (uintptr_t)base + p.offset * sample_bytes, *hi = (uintptr_t)base + end;
    return true;
}

inline bool ranges_overlap(uintptr_t a0, uintptr_t a1, uintptr_t b0, uintptr_t b1) { return a0 < b1 && b0 < a1; }

// ---- B frames of H x W: the shape every format conversion takes (a grid row per frame row); H * W stays below 2^47
inline const char* check_frame_shape(int B, int H, int W)
{
    return B < 1 || H < 1 || W < 1 || B > 65535 || H > 65535 ? "bad frame shape" : nullptr;
}

constexpr size_t kLayoutMax = (size_t)1 << 40;   // a caller's pitch, offset or stride: its products with H stay in range

// A semi-planar surface in samples (NULL or zero fields = tight) -> the resolved one, refused where it cannot hold an
// H x W luma plane and, behind it, `chroma_rows` rows of ceil(W/2) interleaved pairs (NV12 / P010: ceil(H/2) rows;
// p210le: H).  H and W have passed check_frame_shape; chroma_rows is 1..H.
inline const char* resolve_surface(const fiunet_surface_layout* l, int H, int W, size_t chroma_rows, fiunet_surface_layout* out)
{
    const size_t pairs = 2 * (((size_t)W + 1) / 2), luma = (size_t)H * (size_t)W;
    *out = {l && l->luma_pitch ? l->luma_pitch : (size_t)W, l && l->chroma_offset ? l->chroma_offset : luma,
            l && l->chroma_pitch ? l->chroma_pitch : pairs, l && l->frame_stride ? l->frame_stride : luma + chroma_rows * pairs};
    if (std::max({out->luma_pitch, out->chroma_offset, out->chroma_pitch, out->frame_stride}) > kLayoutMax)
        return "surface layout: a value above 2^40 samples";
    if (out->luma_pitch < (size_t)W) return "surface layout: luma_pitch < W";
    if (out->chroma_pitch < pairs) return "surface layout: chroma_pitch < 2*ceil(W/2)";
    if (out->chroma_offset < (size_t)(H - 1) * out->luma_pitch + (size_t)W) return "surface layout: chroma_offset inside the luma plane";
    if (out->frame_stride < out->chroma_offset + (chroma_rows - 1) * out->chroma_pitch + pairs)
        return "surface layout: frame_stride does not cover the chroma plane";
    return nullptr;
}

// One-plane frames in bytes (NULL or zero fields = tight) -> the resolved layout, refused where it cannot hold H rows of
// `row` bytes (packed RGB: W * bpp; y210le: 4 * W; v210: 128 per 48 pixels).  H has passed check_frame_shape.
inline const char* resolve_rows(const fiunet_packed_layout* l, int H, size_t row, fiunet_packed_layout* out)
{
    out->row_pitch = l && l->row_pitch ? l->row_pitch : row;
    if (out->row_pitch > kLayoutMax) return "packed layout: a value above 2^40 bytes";
    out->frame_stride = l && l->frame_stride ? l->frame_stride : (size_t)H * out->row_pitch;
    if (out->frame_stride > kLayoutMax) return "packed layout: a value above 2^40 bytes";
    if (out->row_pitch < row) return "packed layout: row_pitch below the tight row";
    if (out->frame_stride < (size_t)(H - 1) * out->row_pitch + row) return "packed layout: frame_stride does not cover the last row";
    return nullptr;
}

// n >= 1 images of H >= 1 rows of `row` >= 1 samples (W; W * S interleaved; (W - 1) * step + 1 stepped) of `bits` bits,
// rows row_pitch and images image_stride samples apart, at a and b; 10-bit samples are 16-bit words.  The reason lacks its
// subject: the caller puts "frame layout: " or "plane layout: " in front.
inline const char* check_pitched(int bits, int n, int H, size_t row, size_t image_stride, size_t row_pitch, const void* a, const void* b)
{
    if (bits != 8 && bits != 10) return "bits must be 8 or 10";
    if (row_pitch < row) return "row_pitch < W";
    if (row_pitch > kLayoutMax || image_stride > kLayoutMax) return "a value above 2^40 samples";
    // (at most 2^40, image_stride is too small for an image that needs more: H - 1 pitches are multiplied only below that)
    if (n > 1 && ((H > 1 && row_pitch > (kLayoutMax - row) / (size_t)(H - 1)) || image_stride < (size_t)(H - 1) * row_pitch + row))
        return "image_stride smaller than one image";
    if (bits == 10 && ((((uintptr_t)a | (uintptr_t)b) & 1) != 0)) return "10-bit samples are 16-bit words: odd address";
    return nullptr;
}

}  // namespace fiunet
