// conv_common.hip.h -- what the conv kernels (conv3x3_mfma.hip.h, conv3x3_kwave.hip.h), the pointwise kernels
// (pointwise.hip.h) and the host code that launches them share: ConvArgs, the gather modes and epilogues, the element
// traits, the tile geometry (ConvTile, conv_occupancy) and the device helpers of the gather and the epilogue.  No kernel
// is defined here; conv3x3_mfma.hip.h describes the design.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

namespace fiunet {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

enum SrcMode { SRC_DIRECT = 0, SRC_POOL = 1 /* host-side tag only */, SRC_CONCAT_UP = 2,
               SRC_STEM = 3 /* input = stem conv of the raw frame pair, computed in the gather */,
               // precision "bf16x2" (the fp32 contract on the bf16 pipe): direct sources whose activations are TWO bf16
               // pieces, x = hi + lo (16 significant bits), stored [hi planes | lo planes] (4 B per element, fp32's
               // traffic), weights [wh planes | wl planes]; a product is wh*xh + wl*xh + wh*xl with fp32 accumulation
               // (the dropped wl*xl term is 2^-16 relative).  The K loop runs three "virtual planes" per real plane of 32
               // channels - (xh, wh), (xh, wl), (xl, wh) - and the second one reuses the in-tile of the first: every piece
               // is stored once and gathered once.  Every epilogue of this mode writes the two pieces of its output.
               SRC_DIRECT_X2 = 4,
               // bf16x2 + fused stem (gray): the stem conv is evaluated inside the gather as in SRC_STEM, once for the hi
               // piece and once more for the lo piece of each of its two 32-channel planes (same split-bf16 MFMAs, ~2^-16
               // relative: this precision's own accuracy class); the 64-channel two-piece stem output never goes to HBM
               SRC_STEM_X2 = 5 };
constexpr bool src_is_stem(int mode) { return mode == SRC_STEM || mode == SRC_STEM_X2; }
constexpr bool src_is_x2(int mode) { return mode == SRC_DIRECT_X2 || mode == SRC_STEM_X2; }

// Activation layout in HBM: plane-major blocked channels-last, [B][C/PL][H][W][PL] with one
// 64-byte "plane" record per pixel (PL = 32 bf16 / 16 fp32 channels).  A tile row of one plane is
// one contiguous run of (TW+2)*64 bytes, so the LDS-DMA gather of a plane touches every 128-B line
// once and in full (with plain NHWC the two 64-B halves of a 64-channel pixel were fetched by two
// gathers microseconds apart and the line was re-read from HBM when the store stream had evicted
// it).  Byte offset of (plane, y, x) inside one image:
__device__ __forceinline__ size_t blk_off(int plane, int y, int x, int H, int W)
{
    return (((size_t)plane * H + y) * W + x) * 64;
}

struct ConvArgs {
    const void* src0;    // [B][C0/PL][H][W][PL]
    const void* src1;    // CONCAT_UP: low-res [B][C1/PL][lowH][lowW][PL], bilinearly upsampled on the fly
    const void* wgt;     // [Cin/PL][9][Cout][PL]  (plane-major, then tap, cout, channel-in-plane)
    const float* scale;  // [Cout]  gamma / sqrt(var + eps)
    const float* shift;  // [Cout]  beta - mean * scale
    void* dst;           // [B][Cout/PL][H][W][PL] or nullptr (fused head only)
    void* pool_dst;      // EPI_POOL: [B][Cout/PL][H/2][W/2][PL], MaxPool2d(2) of dst
    int B, H, W;         // conv input == output spatial size
    int C0, C1, Cout;    // (SRC_DIRECT_X2: REAL channel counts; every tensor then holds its hi planes followed by its lo planes)
    int lowH, lowW;      // CONCAT_UP: spatial size of src1
    int padT, padL;      // CONCAT_UP: F.pad top/left (unet.py:52-53)
    float sy, sx;        // CONCAT_UP: (low-1)/(2*low-1), align_corners=True scale
    // CONCAT_UP on a horizontal band of a taller image (fiunet_forward_strip); un-tiled: 0, 0, lowH
    int upOffY;          //   global row of this tensor's row 0
    int lowOffY;         //   global row of src1's row 0
    int lowHg;           //   rows of the WHOLE image's low-res tensor (padT, sy are global too)
    int tilesX, tilesY, nct;
    int relu;
    // SRC_STEM (bf16, gray): the 2->64 stem conv + BN + ReLU (unet.py:72) is evaluated inside the
    // in-tile gather of the NEXT conv, so its 64-channel output never goes to HBM.
    const float* f1;          // frame1 [B][1][H][W] fp32
    const float* f2;          // frame2
    const void* stem_w;       // [2 (hi, lo)][64 packed rows][32 k] bf16 of w * bn_scale; k = lane group*8 + dx*2 + frame
                              // with lane groups 0, 1, 2 <-> dy = 0, 2, 1; zero for dx = 3; k = 24 (lane group 3) holds
                              // the BatchNorm shift (its operand is 1.0); packed row R <-> cout bf16_row_to_cout(R)
    float dither;             // bf16 stem only: amplitude of the ordered input dither (stem_dither), 0 = off
    // EPI_SPLITK: the K loop (planes) is cut into `ksplit` slices handled by different workgroups; slice s stores its
    // raw fp32 partial sums to kslab[s][tile][wave][fragment][lane]; splitk_finalize_tile_kernel adds the slices in
    // index order (deterministic) on top of the BatchNorm shift and runs the epilogue.
    int ksplit;
    float* kslab;
    unsigned long long* stamp;  // diagnostic builds (-DFIUNET_STAMP / -DFIUNET_CLOCK) only: one 128-B record (16 cycle sums) per wave
    unsigned stamp_cap;         //   records the buffer holds (waves beyond it do not write)
    const float* head_w; // fused 1x1 head: [head_nc][64]
    const float* head_b; // [head_nc]
    float* head_out;     // fp32 NCHW [B][head_nc][H][W]
    // fiunet_forward_u8: the reference's pre/post-processing (model/inference.py:31-35, :54-61) applied where the
    // frames are read and where the output is written, so no fp32 frame buffer exists
    const uint8_t* u1;        // SRC_STEM: uint8 frames [B][1][H][W] instead of f1 / f2 (nullptr: fp32 frames)
    const uint8_t* u2;
    uint8_t* head_out_u8;     // fused head: uint8 NCHW output instead of head_out (nullptr: fp32 logits)
    int head_nc;
    size_t head_img_stride;   // elements from one image of head_out / head_out_u8 to the next (contiguous: head_nc * H * W;
                              // fiunet_forward_u8_strided: the video loop's interleaved destination, every second frame)
};

template <typename T> struct Elem;
template <> struct Elem<float> {
    static constexpr int PL = 16;  // channels per 64-B plane
    static constexpr int NE = 4;   // elements per 16-B chunk
};
template <> struct Elem<__bf16> {
    static constexpr int PL = 32;
    static constexpr int NE = 8;
};
// precision "fp16": the bf16 layout (2-byte elements, 32 channels per plane) with IEEE half values
template <> struct Elem<_Float16> {
    static constexpr int PL = 32;
    static constexpr int NE = 8;
};

// ---- 16-byte chunk helpers -------------------------------------------------------------------
template <typename T> __device__ __forceinline__ void chunk_unpack(const uint4& c, float* f);
template <> __device__ __forceinline__ void chunk_unpack<float>(const uint4& c, float* f)
{
    f[0] = __uint_as_float(c.x); f[1] = __uint_as_float(c.y);
    f[2] = __uint_as_float(c.z); f[3] = __uint_as_float(c.w);
}
template <> __device__ __forceinline__ void chunk_unpack<__bf16>(const uint4& c, float* f)
{
    f[0] = __uint_as_float(c.x << 16); f[1] = __uint_as_float(c.x & 0xffff0000u);
    f[2] = __uint_as_float(c.y << 16); f[3] = __uint_as_float(c.y & 0xffff0000u);
    f[4] = __uint_as_float(c.z << 16); f[5] = __uint_as_float(c.z & 0xffff0000u);
    f[6] = __uint_as_float(c.w << 16); f[7] = __uint_as_float(c.w & 0xffff0000u);
}
template <> __device__ __forceinline__ void chunk_unpack<_Float16>(const uint4& c, float* f)
{
    typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
    const f16x2 a = __builtin_bit_cast(f16x2, c.x), b = __builtin_bit_cast(f16x2, c.y);
    const f16x2 d = __builtin_bit_cast(f16x2, c.z), e = __builtin_bit_cast(f16x2, c.w);
    f[0] = (float)a[0]; f[1] = (float)a[1]; f[2] = (float)b[0]; f[3] = (float)b[1];
    f[4] = (float)d[0]; f[5] = (float)d[1]; f[6] = (float)e[0]; f[7] = (float)e[1];
}
__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi)
{
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
    bf16x2 v = {(__bf16)lo, (__bf16)hi};  // v_cvt_pk_bf16_f32, round-to-nearest-even
    return __builtin_bit_cast(unsigned, v);
}
// The same conversion spelled as a vector convert: always ONE v_cvt_pk_bf16_f32 (with the SLP
// vectoriser off, the two scalar casts above sometimes come out as two converts and a v_perm).
// Not used everywhere: in the fused-head kernels the shorter form lets hipcc hoist all the packs
// ahead of the head's fp32 math, and spill.
__device__ __forceinline__ unsigned pack_bf16x2_pk(float lo, float hi)
{
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
    typedef __attribute__((ext_vector_type(2))) float f32x2;
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{lo, hi}, bf16x2));
}
// fp32 pair -> fp16 pair, round to nearest even (v_cvt_pk_f16_f32; never the round-toward-zero pkrtz form), SATURATED:
// clamped to +-65504 first (one v_med3_f32 each), so that a value beyond the fp16 range becomes the largest finite one
// instead of inf (and a later inf * 0 = NaN).  fp16 subnormals are kept (no denormal flush in this library's flags).
__device__ __forceinline__ unsigned pack_f16x2(float lo, float hi)
{
    typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
    typedef __attribute__((ext_vector_type(2))) float f32x2;
    const float a = __builtin_amdgcn_fmed3f(lo, -65504.0f, 65504.0f), b = __builtin_amdgcn_fmed3f(hi, -65504.0f, 65504.0f);
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a, b}, f16x2));
}
// The 2-byte packing of the element type: the bf16 kernels keep their two spellings (see above), fp16 has one.
template <typename T> __device__ __forceinline__ unsigned pack2(float lo, float hi)
{
    if constexpr (std::is_same_v<T, _Float16>) return pack_f16x2(lo, hi);
    else return pack_bf16x2(lo, hi);
}
template <typename T> __device__ __forceinline__ unsigned pack2_pk(float lo, float hi)
{
    if constexpr (std::is_same_v<T, _Float16>) return pack_f16x2(lo, hi);
    else return pack_bf16x2_pk(lo, hi);
}
template <typename T> __device__ __forceinline__ uint4 chunk_pack(const float* f);
template <> __device__ __forceinline__ uint4 chunk_pack<float>(const float* f)
{
    return make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]),
                      __float_as_uint(f[3]));
}
template <> __device__ __forceinline__ uint4 chunk_pack<__bf16>(const float* f)
{
    return make_uint4(pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]), pack_bf16x2(f[4], f[5]),
                      pack_bf16x2(f[6], f[7]));
}
template <> __device__ __forceinline__ uint4 chunk_pack<_Float16>(const float* f)
{
    return make_uint4(pack_f16x2(f[0], f[1]), pack_f16x2(f[2], f[3]), pack_f16x2(f[4], f[5]),
                      pack_f16x2(f[6], f[7]));
}

typedef __attribute__((ext_vector_type(2))) short s16x2;
__device__ __forceinline__ unsigned pk_max_i16(unsigned a, unsigned b)
{
    const s16x2 x = __builtin_bit_cast(s16x2, a), y = __builtin_bit_cast(s16x2, b);
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(x, y));  // v_pk_max_i16
}

template <typename T>
__device__ __forceinline__ uint4 chunk_max4(const uint4& a, const uint4& b, const uint4& c,
                                            const uint4& d);

// bf16 max-pool of NON-NEGATIVE values (every pooled tensor in this network is a ReLU output):
// for x >= 0 the bf16 order equals the signed 16-bit integer order of the bit patterns, and a
// stray -0.0 (0x8000 = INT16_MIN) loses against everything, so a packed integer max is exact.
template <>
__device__ __forceinline__ uint4 chunk_max4<__bf16>(const uint4& a, const uint4& b, const uint4& c,
                                                    const uint4& d)
{
    return make_uint4(pk_max_i16(pk_max_i16(a.x, b.x), pk_max_i16(c.x, d.x)),
                      pk_max_i16(pk_max_i16(a.y, b.y), pk_max_i16(c.y, d.y)),
                      pk_max_i16(pk_max_i16(a.z, b.z), pk_max_i16(c.z, d.z)),
                      pk_max_i16(pk_max_i16(a.w, b.w), pk_max_i16(c.w, d.w)));
}

// fp16: the same integer max - for x >= 0 the fp16 order is the int16 order of the bit patterns too
template <>
__device__ __forceinline__ uint4 chunk_max4<_Float16>(const uint4& a, const uint4& b, const uint4& c,
                                                      const uint4& d)
{
    return chunk_max4<__bf16>(a, b, c, d);
}

template <>
__device__ __forceinline__ uint4 chunk_max4<float>(const uint4& a, const uint4& b, const uint4& c,
                                                   const uint4& d)
{
    using T = float;
    constexpr int NE = Elem<T>::NE;
    float fa[NE], fb[NE], fc[NE], fd[NE], r[NE];
    chunk_unpack<T>(a, fa); chunk_unpack<T>(b, fb); chunk_unpack<T>(c, fc); chunk_unpack<T>(d, fd);
#pragma unroll
    for (int i = 0; i < NE; ++i) r[i] = fmaxf(fmaxf(fa[i], fb[i]), fmaxf(fc[i], fd[i]));
    return chunk_pack<T>(r);  // exact for bf16: the max is one of the (bf16) inputs
}

// hy*(hx*a + lx*b) + ly*(hx*c + lx*d): the association aten's upsample_bilinear2d uses.
template <typename T>
__device__ __forceinline__ uint4 chunk_bilerp(const uint4& a, const uint4& b, const uint4& c,
                                              const uint4& d, float hx, float lx, float hy,
                                              float ly)
{
    constexpr int NE = Elem<T>::NE;
    float fa[NE], fb[NE], fc[NE], fd[NE], r[NE];
    chunk_unpack<T>(a, fa); chunk_unpack<T>(b, fb); chunk_unpack<T>(c, fc); chunk_unpack<T>(d, fd);
    // explicit fma pattern: the same bits in every kernel this is inlined into (hipcc's default
    // fp-contract=fast would otherwise pick a different contraction per context)
#pragma unroll
    for (int i = 0; i < NE; ++i) {
        const float top = fmaf(lx, fb[i], __fmul_rn(hx, fa[i]));
        const float bot = fmaf(lx, fd[i], __fmul_rn(hx, fc[i]));
        r[i] = fmaf(ly, bot, __fmul_rn(hy, top));
    }
    return chunk_pack<T>(r);
}

// The two halves of chunk_bilerp, for callers that walk down a column and reuse the horizontal
// result of a low-res row for every output row that touches it.  Same operations on the same
// operands in the same order as chunk_bilerp, hence the same bits.
template <typename T>
__device__ __forceinline__ void chunk_hlerp(const uint4& a, const uint4& b, float hx, float lx, float* h)
{
    constexpr int NE = Elem<T>::NE;
    float fa[NE], fb[NE];
    chunk_unpack<T>(a, fa); chunk_unpack<T>(b, fb);
#pragma unroll
    for (int i = 0; i < NE; ++i) h[i] = fmaf(lx, fb[i], __fmul_rn(hx, fa[i]));
}
template <typename T>
__device__ __forceinline__ uint4 chunk_vlerp(const float* top, const float* bot, float hy, float ly)
{
    constexpr int NE = Elem<T>::NE;
    float r[NE];
#pragma unroll
    for (int i = 0; i < NE; ++i) r[i] = fmaf(ly, bot[i], __fmul_rn(hy, top[i]));
    return chunk_pack<T>(r);
}


__device__ __forceinline__ uint4 ldg16(const char* p) { return *reinterpret_cast<const uint4*>(p); }

// model/inference.py:31-35: image.astype(float32) / 255.0 ; 2.0 * image - 1.0   (numpy fp32 arithmetic)
__device__ __forceinline__ float preprocess_u8_value(unsigned char u)
{
    // u / 255 correctly rounded without the division sequence: q0 = u * RN(1/255), one Newton correction
    // with the exact remainder (fma); equal to the IEEE quotient for all 256 codes (asserted bit for bit
    // against numpy by tests/test_gpu_parity.py over every code)
    const float x = (float)u, r = 1.0f / 255.0f;
    const float q0 = __fmul_rn(x, r);
    const float q = fmaf(fmaf(-q0, 255.0f, x), r, q0);
    return __fsub_rn(__fmul_rn(2.0f, q), 1.0f);
}
// model/inference.py:54-61: (x + 1) / 2 ; clamp(0, 1) ; (x * 255).astype(uint8) -- truncation
__device__ __forceinline__ unsigned char postprocess_u8_value(float x)
{
    float v = __fdiv_rn(__fadd_rn(x, 1.0f), 2.0f);
    v = fminf(fmaxf(v, 0.0f), 1.0f);
    return (unsigned char)(int)__fmul_rn(v, 255.0f);
}

// Ordered dither of the bf16 path's INPUT (bf16 stem only; the fp32 path never sees it).
// Why: a bf16 activation has 8 significant bits, the frames have 8 too (x = 2*u8/255 - 1), and a network
// that interpolates carries the frames themselves through the full-resolution skip (x1 -> up4).  Rounded
// to nearest, the error of such a carried value is a fixed sawtooth of the pixel's intensity, i.e. a
// small intensity-dependent gain/offset error that is the same in every smooth region of the image: it
// correlates with the content and moves PSNR-vs-truth by 0.03-0.05 dB on an interpolating checkpoint,
// ten times what its energy alone would (tools/bf16_emulate.py isolates it: rounding the stem output /
// x1 / up4.0 accounts for nearly all of the bf16 path's PSNR difference; all other layers together for
// < 0.01 dB).  The classic remedy is dither: frame 1 gets +d(y, x), frame 2 gets -d(y, x) before the
// stem conv, d = the 8x8 Bayer matrix scaled to a quarter of an 8-bit input step peak-to-peak/2
// (amplitude 2^-8 = +-2^-9, below the frames' own quantisation noise).  The rounding error of a carried
// value then averages to zero over every 8x8 block whatever the intensity, and in the blend
// 0.5*(f1 + f2) the two dithers cancel exactly.  Measured (emulation, 5 checkpoints x 5 scenes):
// |PSNR_bf16 - PSNR_fp32| 0.017-0.039 dB -> <= 0.0125 dB, rel-L2 of the output error slightly lower.
// Deterministic and position-based: (y & 7, x & 7) of the GLOBAL pixel (strip origins are multiples of
// 16 rows), so tiled == un-tiled and batch invariance are unaffected.
__device__ __forceinline__ float stem_dither(int y, int x)
{
    // Bayer index matrix M8: bits of (x ^ y) and y interleaved, bit 0 most significant
    const unsigned a = (unsigned)(x ^ y) & 7u, b = (unsigned)y & 7u;
    const unsigned m = ((a & 1u) << 5) | ((b & 1u) << 4) | ((a & 2u) << 2) | ((b & 2u) << 1) | ((a & 4u) >> 1) | ((b & 4u) >> 2);
    return ((float)m + 0.5f) * (1.0f / 64.0f) - 0.5f;  // (-0.5, 0.5), 64 levels, zero mean over a period
}

// Bilinear x2 (align_corners=True) source coordinates and weights of one upsampled+padded pixel
// (unet.py:40,49-53), shared by every kernel that upsamples so they agree bit for bit.
struct UpAxis {
    int i0, i1;   // low-res source indices (local to the tensor at hand)
    float h, l;   // weights of i0, i1
    bool ok;      // inside the upsampled extent (false: F.pad zero)
};
// One axis of the mapping.  c = conv-input coordinate (already clamped to the local tensor).
// Strip-tiled forwards (fiunet_forward_strip) run on a horizontal band of a taller image: the
// mapping is then evaluated in GLOBAL coordinates (c + off; low-res extent lowNg; pad and scale of
// the whole image) and only the resulting source indices are moved back into the band (- lowOff,
// clamped to its lowN rows), so a band computes exactly what the whole image would.  Un-tiled:
// off = lowOff = 0 and lowNg = lowN.
__device__ __forceinline__ UpAxis up_axis(int c, int off, int pad, int lowNg, float scale, int lowOff,
                                          int lowN)
{
    UpAxis u;
    int cu = c + off - pad;
    u.ok = (cu >= 0) & (cu < 2 * lowNg);
    cu = min(max(cu, 0), 2 * lowNg - 1);
    // f is the ROUNDED product, as in aten (the library is built with -ffp-contract=off)
    const float f = scale * (float)cu;
    const int g0 = (int)f;
    const int g1 = g0 < lowNg - 1 ? g0 + 1 : g0;
    u.l = f - (float)g0;
    u.h = 1.0f - u.l;
    u.i0 = min(max(g0 - lowOff, 0), lowN - 1);
    u.i1 = min(max(g1 - lowOff, 0), lowN - 1);
    return u;
}
__device__ __forceinline__ UpAxis up_axis_y(const ConvArgs& a, int y)
{
    return up_axis(y, a.upOffY, a.padT, a.lowHg, a.sy, a.lowOffY, a.lowH);
}
__device__ __forceinline__ UpAxis up_axis_x(const ConvArgs& a, int x)
{
    return up_axis(x, 0, a.padL, a.lowW, a.sx, 0, a.lowW);
}
struct UpCoord {
    int y0, y1, x0, x1;
    float hy, ly, hx, lx;
    bool ok;
};
__device__ __forceinline__ UpCoord up_coord(const ConvArgs& a, int y, int x)
{
    const UpAxis v = up_axis_y(a, y), h = up_axis_x(a, x);
    UpCoord u;
    u.y0 = v.i0; u.y1 = v.i1; u.hy = v.h; u.ly = v.l;
    u.x0 = h.i0; u.x1 = h.i1; u.hx = h.h; u.lx = h.l;
    u.ok = v.ok & h.ok;
    return u;
}

// One 16-byte chunk (plane `plane`, chunk `ch`) of conv-input pixel (b, y, x) straight from
// global memory; zero outside the image (conv padding) and outside the upsampled extent (F.pad).
// Used by the standalone (ablation) upsample+concat kernel; the fused conv computes the same
// values from an LDS-staged low-res tile.
template <typename T, int MODE>
__device__ __forceinline__ uint4 gather_chunk(const ConvArgs& a, int b, int y, int x, int plane,
                                              int ch)
{
    constexpr int PL = Elem<T>::PL;
    bool ok = (y >= 0) & (y < a.H) & (x >= 0) & (x < a.W);
    y = min(max(y, 0), a.H - 1);
    x = min(max(x, 0), a.W - 1);
    const int p0 = a.C0 / PL;
    uint4 v;
    if (MODE == SRC_DIRECT || plane < p0) {
        const char* p = (const char*)a.src0 + (size_t)b * a.H * a.W * a.C0 * sizeof(T) +
                        blk_off(plane, y, x, a.H, a.W) + ch * 16;
        v = ldg16(p);
    } else {
        const UpCoord u = up_coord(a, y, x);
        ok = ok & u.ok;
        const char* base = (const char*)a.src1 + (size_t)b * a.lowH * a.lowW * a.C1 * sizeof(T) + ch * 16;
        const int q = plane - p0;
        const uint4 v00 = ldg16(base + blk_off(q, u.y0, u.x0, a.lowH, a.lowW));
        const uint4 v01 = ldg16(base + blk_off(q, u.y0, u.x1, a.lowH, a.lowW));
        const uint4 v10 = ldg16(base + blk_off(q, u.y1, u.x0, a.lowH, a.lowW));
        const uint4 v11 = ldg16(base + blk_off(q, u.y1, u.x1, a.lowH, a.lowW));
        v = chunk_bilerp<T>(v00, v01, v10, v11, u.hx, u.lx, u.hy, u.ly);
    }
    return ok ? v : make_uint4(0u, 0u, 0u, 0u);
}

// LDS-DMA: 16 bytes per lane, global -> LDS, destination = wave-uniform LDS byte address (in M0)
// + lane*16.  Issued from inline asm ON PURPOSE: hipcc treats the builtin form as an LDS store
// that may alias every later ds_read and drains it with s_waitcnt vmcnt(0) before the first
// fragment read of the step, which would serialise the weight stream with the MFMAs.  The asm
// form is invisible to its wait bookkeeping, so completion is waited for by hand
// (lds_dma_wait_all) before the barrier that publishes the data.  M0 is saved/restored in
// the same statement (cdna_hip_programming.md 5.7).
__device__ __forceinline__ void glds16(const char* gsrc, unsigned lds_wave_base)
{
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gsrc), "s"(lds_wave_base)
                 : "memory");
}
// The same with a wave-uniform 64-bit base in SGPRs and a 32-bit per-lane byte offset: one VGPR per
// address instead of two.  Lanes switched off by EXEC neither load nor write their 16 LDS bytes.
__device__ __forceinline__ void glds16s(const char* sbase, unsigned voff, unsigned lds_wave_base)
{
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(sbase), "s"(lds_wave_base)
                 : "memory");
}
__device__ __forceinline__ void lds_dma_wait_all() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
__device__ __forceinline__ unsigned lds_addr_of(const char* p)
{
    return (unsigned)(uintptr_t)(__attribute__((address_space(3))) const char*)p;
}

__device__ __forceinline__ int swz(int row) { return ((row >> 2) & 1) << 1; }

template <typename T>
__device__ __forceinline__ void mma_chunk(f32x4& acc, const uint4& wa, const uint4& xb);
template <>
__device__ __forceinline__ void mma_chunk<__bf16>(f32x4& acc, const uint4& wa, const uint4& xb)
{
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wa),
                                                  __builtin_bit_cast(bf16x8, xb), acc, 0, 0, 0);
}
template <>
__device__ __forceinline__ void mma_chunk<_Float16>(f32x4& acc, const uint4& wa, const uint4& xb)
{
    // the same shape, operand layout (8 values per lane, k-slots lane group*8 .. +7) and rate as the bf16 instruction
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, wa),
                                                 __builtin_bit_cast(f16x8, xb), acc, 0, 0, 0);
}
template <>
__device__ __forceinline__ void mma_chunk<float>(f32x4& acc, const uint4& wa, const uint4& xb)
{
    // lane group g = lane>>4 holds channels 4g..4g+3 of the plane in both operands; MFMA i
    // consumes element i of every group, i.e. k-slot g <-> channel 4g+i on both sides.
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(wa.x), __uint_as_float(xb.x), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(wa.y), __uint_as_float(xb.y), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(wa.z), __uint_as_float(xb.z), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(wa.w), __uint_as_float(xb.w), acc, 0, 0, 0);
}

enum Epilogue { EPI_PLAIN = 0, EPI_HEAD = 1 /* 1x1 head, 1 class */, EPI_POOL = 2, EPI_HEAD3 = 3 /* 3 classes */,
                EPI_SPLITK = 4 /* raw fp32 partial sums of a K slice -> slab (small problems); splitk_finalize_tile_kernel reduces */ };
constexpr bool epi_is_splitk(int epi) { return epi == EPI_SPLITK; }

// value of the neighbouring lane (lane ^ 1) through DPP quad_perm [1,0,3,2]: no LDS crossbar
__device__ __forceinline__ unsigned dpp_swap_pairs(unsigned v)
{
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);
}

// number of row segments for the column-walk upsample (see gather_plane_up): minimise
// passes over the 256 threads x (rows per segment + ~1 row of segment start-up)
constexpr int up_segments(int rows, int ncol)
{
    int best = 1, best_cost = 1 << 30;
    for (int n = 1; n <= 6; ++n) {
        const int passes = (n * ncol + 255) / 256, segr = (rows + n - 1) / n;
        const int cost = passes * (segr * 4 + 3);
        if (cost < best_cost) { best_cost = cost; best = n; }
    }
    return best;
}

// LDS map of one workgroup (<= 80 KiB so that two fit on a CU):
//   [ in-tile | W slot 0 | spare | W slot 1 ]
// The spare region sits between the two ring slots so that, whichever slot is idle at a plane
// boundary, idle slot + spare form one contiguous staging area for the low-res tile of an
// upsampled plane.
template <int BN, int TH, int TW, int MODE> struct ConvTile {
    static constexpr int TWP = ((TW + 2 + 7) / 8) * 8;  // in-tile row pitch, multiple of 8 pixels
    static constexpr int THP = TH + 2;
    static constexpr int IN_BYTES = THP * TWP * 64;
    static constexpr int W_BYTES = 3 * BN * 64;          // one (plane, kx) step: 3 taps
    // low-res tile of an upsampled plane: rows/cols that a (TH+2)x(TW+2) window can touch
    static constexpr int LRH = (TH + 1) / 2 + 3, LRW = (TW + 1) / 2 + 3, LRP = ((LRW + 3) / 4) * 4;
    static constexpr int LR_PIECES = (LRH * LRP + 15) / 16;
    // spare bytes between the ring slots: only what the staging area needs beyond one slot
    static constexpr int SPARE_BYTES =
        (MODE == SRC_CONCAT_UP && LR_PIECES * 1024 > W_BYTES) ? LR_PIECES * 1024 - W_BYTES : 0;
    static constexpr int W_STRIDE = W_BYTES + SPARE_BYTES;  // slot 1 = slot 0 + W_STRIDE
    // (Two ring slots.  A 4-deep ring for the small tiles - W(step+3) requested at the top of `step`, counted waits - was built in
    // round 6 and measured NULL on the small problems it was meant for (a lone workgroup's step is issue / LDS latency, not L2
    // latency: profiles/r06_cfg_sweep_b1_256_bf16_first_version.txt against r06_cfg_sweep_b1_256_bf16.txt), and its 24 KiB cost the
    // small tile its third workgroup per CU, which IS worth 5-17 % on the deep levels of one to four 1080p pairs.)
    // SRC_STEM: raw patch of both frames, (TH+4) x (TW+4) pixels, after the ring: bf16 dwords {frame1,
    // frame2}, the hi and the lo part of a patch row side by side, [row][hi | lo][PATCH_W].  The row pitch
    // of 2 * PATCH_W = 72 dwords makes rows py and py+2 - read together by lane groups 0 and 1 of a
    // ds_read2_b32 (lanes 0-31, 32 banks) - sit 144 = 16 (mod 32) banks apart: no conflicts (separate hi
    // and lo images of pitch 36 put rows py, py+1 only 4 banks apart: 2-way conflicts on 12 of 16 lanes).
    static constexpr int PATCH_W = TW + 4, PATCH_H = TH + 4, PATCH_PITCH = 2 * PATCH_W;
    static_assert(!src_is_stem(MODE) || (2 * PATCH_PITCH) % 32 == 16, "patch pitch: lane groups 0/1 must not share banks");
    static constexpr int PATCH_OFF = IN_BYTES + 2 * W_BYTES + SPARE_BYTES;
    // The operand of the bias k-slot - PATCH_W dwords {1.0, 0} followed by PATCH_W zero dwords (its lo
    // part), which all lanes of lane group 3 read at the same address (a broadcast) - lives in the
    // row-pitch filler of in-tile row 0 (pixels TW+2 .. TWP-1: never written or read in this mode), so
    // that the workgroup stays at 63 LDS allocation granules of 1280 B: at 64 (= 80 KiB, two workgroups
    // filling the CU's LDS exactly) this kernel ran 5 % slower.
    static constexpr int PATCH_TAIL_OFF = (TW + 2) * 64;                 // byte offset inside the in-tile
    static constexpr int PATCH_TAIL = 2 * PATCH_W * 4;
    static_assert(!src_is_stem(MODE) || PATCH_TAIL_OFF + PATCH_TAIL <= TWP * 64, "bias operand must fit the row-pitch filler");
    static constexpr int PATCH_BYTES = src_is_stem(MODE) ? PATCH_H * PATCH_PITCH * 4 : 0;
    // CONCAT_UP: the bilinear mapping of this tile, one 16-B entry per in-tile row and per in-tile
    // pixel column (same for every plane, so it is evaluated once per tile, not per plane)
    static constexpr int TAB_OFF = PATCH_OFF + ((PATCH_BYTES + 15) / 16) * 16;
    static constexpr int TAB_BYTES = MODE == SRC_CONCAT_UP ? ((THP + TW + 2) * 16 + 255) / 256 * 256 : 0;
    // SRC_STEM: plane 1's stem weights (hi and lo halves of two 16-cout tiles), parked here by
    // LDS-DMA at kernel start so the plane boundary does not wait on a global load
    static constexpr int STEMW_OFF = TAB_OFF + TAB_BYTES;
    static constexpr int STEMW_BYTES = src_is_stem(MODE) ? 4096 : 0;
    static constexpr int LDS_BYTES = STEMW_OFF + STEMW_BYTES;
    static_assert(LDS_BYTES <= 80 * 1024, "two workgroups must fit in the CU's 160 KiB of LDS");
    static_assert(!src_is_stem(MODE) || LDS_BYTES <= 63 * 1280, "fused-stem kernel: stay below 64 LDS granules");
};

// 16-pixel fragments per wave: 8 (wave tile 64 couts x 128 pixels, 128 accumulator registers, two
// workgroups per CU) or 4 (64 x 64, 64 accumulator registers, three workgroups per CU: for the
// short-K full-resolution layers, whose prologue/epilogue share is large, a third resident wave per
// SIMD keeps the MFMA pipe fed while the other two gather or store).
constexpr int conv_wave_frags(int BN, int TH, int TW) { return TH * TW / 16 / (4 / (BN / 64)); }
// (a 64 x 64 wave tile whose workgroup needs more than a third of the CU's LDS - the fused-stem gather - stays at two)
constexpr int conv_occupancy(int BN, int TH, int TW, int lds_bytes = 0)
{
    return conv_wave_frags(BN, TH, TW) == 4 && lds_bytes * 3 <= 160 * 1024 ? 3 : 2;
}

// ---- tile indexing, accumulator set-up and epilogue shared by the conv kernels -----------------

// XCD-aware, bijective block remap: blocks sharing an input tile (different cout tiles) and neighbouring
// tiles get consecutive logical ids on ONE XCD so the re-reads hit its L2.
__device__ __forceinline__ int conv_block_remap()
{
    const int nblk = gridDim.x, bid = blockIdx.x;
    const int q = nblk >> 3, r = nblk & 7, xcd = bid & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

// Logical tile index -> (cout tile, image, tile row, tile column); the cout tile varies fastest.
struct ConvTileId { int ct, b, ty, tx; };
__device__ __forceinline__ ConvTileId conv_tile_decode(const ConvArgs& a, int t)
{
    ConvTileId d;
    d.ct = t % a.nct; t /= a.nct;
    d.tx = t % a.tilesX; t /= a.tilesX;
    d.ty = t % a.tilesY;
    d.b = t / a.tilesY;
    return d;
}

// Eval-mode BatchNorm is folded on both sides of the K loop: its scale into the packed weights
// (fiunet_load_weights) and its shift into the INITIAL value of the accumulators, so the epilogue is
// just y = relu(acc).  Which couts a lane holds: accumulator tile m, register j of lane group lc is
// MFMA row lc*4+j of that tile.  fp32: row r of tile m <-> cout m*16+r, so a lane's 4 registers are
// one 16-B quarter of the tile's 64-B plane record.  bf16: the packed weight rows are permuted on the
// host (fiunet.hip, `bf16_row_to_cout`) so that tiles 2g and 2g+1 together give the lane the 8
// consecutive couts g*32+lc*8 .. +7: ONE 16-B store per lane and tile pair, and the 4 lane groups of
// a pixel write its whole 64-B record (1 KiB contiguous per store instruction).
template <typename T> __device__ __forceinline__ int conv_cout_ofs(int m, int lc)
{
    return sizeof(T) == 2 ? (m >> 1) * 32 + lc * 8 + (m & 1) * 4 : m * 16 + lc * 4;  // cout (within the wave) of register j = 0
}

template <typename T, int BN, int TH, int TW, int EPI>
__device__ __forceinline__ void conv_acc_init(const ConvArgs& a, f32x4 (&acc)[4][conv_wave_frags(BN, TH, TW)],
                                              int ct, int wc, int lc)
{
    constexpr int NF = conv_wave_frags(BN, TH, TW);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (!epi_is_splitk(EPI)) {  // K slices start from zero; the reduction adds the shift
            const float4 sh = *reinterpret_cast<const float4*>(a.shift + ct * BN + wc * 64 + conv_cout_ofs<T>(m, lc));
            v = f32x4{sh.x, sh.y, sh.z, sh.w};
        }
#pragma unroll
        for (int n = 0; n < NF; ++n) acc[m][n] = v;
    }
}

// bf16 pair -> relu on the packed pair: for x < 0 (sign bit set, incl. -0.0) the int16 pattern is negative
// (the same holds for an fp16 pair: the fp16 kernels use it too)
__device__ __forceinline__ unsigned relu_pk_bf16(unsigned p) { return pk_max_i16(p, 0u); }
// sum += max(x, lo) * w: v_max_f32 + v_fmac_f32 as one block (fmaxf() costs a canonicalising
// v_max(x, x) in front, and a lone inline-asm v_max an s_nop behind)
__device__ __forceinline__ void relu_fma(float& sum, float x, float lo, float w)
{
    float t;
    asm("v_max_f32 %1, %3, %2\n\tv_fmac_f32 %0, %1, %4" : "+v"(sum), "=&v"(t) : "v"(x), "v"(lo), "v"(w));
}

//      y = relu(acc) -> blocked activation records (+ fused pool / head / split-K slab).  acc[m][n]:
//      accumulator tile m (16 couts) x pixel fragment n of the wave (wc = cout half, wp = pixel
//      group) of workgroup tile (b, y0, x0), cout tile ct, K slice `split`.
template <typename T, int BN, int TH, int TW, int EPI, bool X2 = false>
__device__ __forceinline__ void conv_epilogue(const ConvArgs& a, f32x4 (&acc)[4][conv_wave_frags(BN, TH, TW)],
                                              int b, int y0, int x0, int ct, int split, int wc, int wp,
                                              int l15, int lc)
{
    constexpr int PL = Elem<T>::PL;
    constexpr int FR = TW / 16;
    constexpr int NF = conv_wave_frags(BN, TH, TW);
    constexpr int ROWS_W = NF / FR;
    constexpr int HNC = EPI == EPI_HEAD ? 1 : (EPI == EPI_HEAD3 ? 3 : 0);
    const int aH = a.H, aW = a.W;
    constexpr bool PERM = sizeof(T) == 2;
    const int wbase_c = ct * BN + wc * 64;  // first cout of this wave
    if constexpr (epi_is_splitk(EPI)) {
        // raw fp32 partial sums of this K slice, in FRAGMENT order: slab[split][tile][wave][m * NF + n][lane] as float4,
        // so every store instruction of a wave writes 1 KiB contiguous (round 6; the pixel-major slab of rounds 1-5 was
        // written 16 B at a time with a stride of Cout floats: 29 % of a K-split kernel's wave time was this epilogue,
        // profiles/r06_stamp_phases_b1_256_before_small_tiles.txt).  splitk_finalize_tile_kernel reads it back in the same order.
        const int tile = (((b * a.tilesY) + y0 / TH) * a.tilesX + x0 / TW) * a.nct + ct;
        const int ntile = a.B * a.tilesY * a.tilesX * a.nct;
        const int wave = wp * (BN / 64) + wc;
        float4* o = reinterpret_cast<float4*>(a.kslab) + ((((size_t)split * ntile + tile) * 4 + wave) * (4 * NF)) * 64 + (lc * 16 + l15);
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < NF; ++n)
                o[(m * NF + n) * 64] = make_float4(acc[m][n][0], acc[m][n][1], acc[m][n][2], acc[m][n][3]);
        return;
    }
    float hw[HNC > 0 ? HNC : 1][4][4];
#pragma unroll
    for (int c = 0; c < HNC; ++c)
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const float4 v = *reinterpret_cast<const float4*>(a.head_w + c * 64 + conv_cout_ofs<T>(m, lc));
            hw[c][m][0] = v.x; hw[c][m][1] = v.y; hw[c][m][2] = v.z; hw[c][m][3] = v.w;
        }
    // record address = image base + plane * plane_stride + pixel * 64 + byte within the record
    const size_t plane_stride = (size_t)aH * aW * 64;
    const int plane0 = wbase_c / PL;                       // first output plane of this wave
    const int rec_byte = lc * 16;                          // this lane's 16 B of a 64-B record
    char* const out_img = a.dst ? (char*)a.dst + (size_t)b * plane_stride * (a.Cout / PL) +
                                  (size_t)plane0 * plane_stride + rec_byte : nullptr;
    const int pH = aH >> 1, pW = aW >> 1;  // EPI_POOL: MaxPool2d(2) output size (floor)
    const size_t pplane_stride = (size_t)pH * pW * 64;
    char* const pool_img = EPI == EPI_POOL ? (char*)a.pool_dst + (size_t)b * pplane_stride * (a.Cout / PL) +
                                             (size_t)plane0 * pplane_stride + rec_byte : nullptr;
    if constexpr (HNC > 0) {
        // Fused 1x1 head on the fp32 post-activation values (never rounded to bf16).  Every lane sums
        // its 16 couts for each of the 8 fragments; the four lane groups of a pixel are then combined
        // by a transposing reduction (v_permlane16_swap / v_permlane32_swap: 6 swaps instead of 16
        // bpermutes, same (lc0 + lc1) + (lc2 + lc3) order), which leaves fragments nb, nb + 1 complete
        // in lane group lc: all 64 lanes store, 2 dwords each.
        static_assert(HNC == 0 || NF == 8 || NF == 4, "head reduction is written for 8 or 4 fragments per wave");
        const float floor_v = a.relu ? 0.f : -__builtin_inff();
        float hb[HNC];
#pragma unroll
        for (int c = 0; c < HNC; ++c) hb[c] = a.head_b[c];
        const int nb = ((lc & 1) ? 4 : 0) + ((lc & 2) ? 2 : 0);
#pragma unroll
        for (int c = 0; c < HNC; ++c) {
            float hs[NF];
#pragma unroll
            for (int n = 0; n < NF; ++n) {
                float sum = 0.f;
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int j = 0; j < 4; ++j) relu_fma(sum, acc[m][n][j], floor_v, hw[c][m][j]);
                hs[n] = sum;
            }
            if constexpr (NF == 4) {
                // 64 x 64 wave tiles (small problems): four fragments, one per lane group after the reduction.  Two
                // xor-shuffles per fragment give every lane (g0 + g1) + (g2 + g3) of its pixel - the association of
                // the transposing reduction below (fp addition commutes), so the output bits do not depend on the tile
                float full[NF];
#pragma unroll
                for (int n = 0; n < NF; ++n) {
                    const float p = hs[n] + __shfl_xor(hs[n], 16);
                    full[n] = p + __shfl_xor(p, 32);
                }
                const float mine = lc == 0 ? full[0] : (lc == 1 ? full[1] : (lc == 2 ? full[2] : full[3]));
                const int n = lc;
                const int y = y0 + wp * ROWS_W + n / FR;
                const int x = x0 + (n % FR) * 16 + l15;
                if (y < aH && x < aW) {
                    const size_t o = (size_t)b * a.head_img_stride + ((size_t)c * aH + y) * aW + x;
                    if (a.head_out_u8) a.head_out_u8[o] = postprocess_u8_value(mine + hb[c]);
                    else a.head_out[o] = mine + hb[c];
                }
            } else {
                float t[4], u[2];
#pragma unroll
                for (int i = 0; i < 4; ++i) {  // rows 0, 2: fragment i; rows 1, 3: fragment i + 4
                    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(hs[i]), __float_as_uint(hs[(i + 4) % NF]), false, false);
                    t[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
                }
#pragma unroll
                for (int j = 0; j < 2; ++j) {  // rows 0, 1: t[j]; rows 2, 3: t[j + 2]
                    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(t[j]), __float_as_uint(t[j + 2]), false, false);
                    u[j] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
                }
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int n = nb + j;
                    const int y = y0 + wp * ROWS_W + n / FR;
                    const int x = x0 + (n % FR) * 16 + l15;
                    if (y < aH && x < aW) {
                        const size_t o = (size_t)b * a.head_img_stride + ((size_t)c * aH + y) * aW + x;
                        if (a.head_out_u8) a.head_out_u8[o] = postprocess_u8_value(u[j] + hb[c]);
                        else a.head_out[o] = u[j] + hb[c];
                    }
                }
            }
        }
    }
    if constexpr (X2) {
        // precision "bf16x2": relu(acc) in fp32 -> two bf16 pieces, stored [hi planes | lo planes] (two 16-B stores per
        // lane and tile pair; a fused-head conv stores only when the read-back keeps its activation)
        static_assert(std::is_same_v<T, __bf16>, "the two-piece epilogue belongs to the bf16 kernels");
        if (HNC > 0 && !a.dst) return;
        const size_t ps = (size_t)aH * aW * 64;                  // bytes of one 32-channel plane
        const int npo = a.Cout / 32;                             // planes per piece; the tensor has 2 * npo
        const size_t blk = (size_t)npo * ps;                     // bytes from the hi piece to the lo piece
        char* const img = (char*)a.dst + (size_t)b * 2 * blk + (size_t)(wbase_c / 32) * ps + lc * 16;
        const int pH2 = aH >> 1, pW2 = aW >> 1;
        const size_t pps = (size_t)pH2 * pW2 * 64, pblk = (size_t)npo * pps;
        char* const pimg = EPI == EPI_POOL ? (char*)a.pool_dst + (size_t)b * 2 * pblk + (size_t)(wbase_c / 32) * pps + lc * 16
                                           : nullptr;
        // 8 consecutive couts of this lane (accumulator tiles 2g, 2g + 1) -> hi and lo chunk
        auto put = [&](char* o, size_t block_bytes, const float (&v)[8]) __attribute__((always_inline)) {
            unsigned h[4], l[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                h[i] = pack_bf16x2_pk(v[2 * i], v[2 * i + 1]);
                l[i] = pack_bf16x2_pk(v[2 * i] - __uint_as_float(h[i] << 16), v[2 * i + 1] - __uint_as_float(h[i] & 0xffff0000u));
            }
            *reinterpret_cast<uint4*>(o) = make_uint4(h[0], h[1], h[2], h[3]);
            *reinterpret_cast<uint4*>(o + block_bytes) = make_uint4(l[0], l[1], l[2], l[3]);
        };
#pragma unroll
        for (int n = 0; n < NF; ++n) {
            const int y = y0 + wp * ROWS_W + n / FR;
            const int x = x0 + (n % FR) * 16 + l15;
            if (y < aH && x < aW) {
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        v[j] = a.relu ? fmaxf(acc[2 * g][n][j], 0.f) : acc[2 * g][n][j];
                        v[4 + j] = a.relu ? fmaxf(acc[2 * g + 1][n][j], 0.f) : acc[2 * g + 1][n][j];
                    }
                    put(img + (size_t)(y * aW + x) * 64 + g * ps, blk, v);
                }
            }
        }
        if constexpr (EPI == EPI_POOL) {
            // MaxPool2d(2) on the fp32 values (relu is monotonic): rows n / n + FR of this wave, column partner = lane ^ 1
#pragma unroll
            for (int n = 0; n < NF; ++n) {
                if (((n / FR) & 1) != 0) continue;
                const int y = y0 + wp * ROWS_W + n / FR;
                const int x = x0 + (n % FR) * 16 + l15;
                const int py = y >> 1, px = x >> 1;
                const bool okp = (py < pH2) && (px < pW2) && ((l15 & 1) == 0);
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    float v[8];
#pragma unroll
                    for (int h = 0; h < 2; ++h)
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float cm = fmaxf(acc[2 * g + h][n][j], acc[2 * g + h][n + FR][j]);
                            float r = fmaxf(cm, __uint_as_float(dpp_swap_pairs(__float_as_uint(cm))));
                            if (a.relu) r = fmaxf(r, 0.f);
                            v[4 * h + j] = r;
                        }
                    if (okp) put(pimg + (size_t)(min(py, pH2 - 1) * pW2 + min(px, pW2 - 1)) * 64 + g * pps, pblk, v);
                }
            }
        }
        return;
    }
    if constexpr (EPI == EPI_POOL && PERM) {
        // bf16 + fused MaxPool2d(2) (unet.py:28): a wave owns whole row pairs (fragments n and n + FR), the
        // column partner is the neighbouring lane (l15 ^ 1).  The packed, relu'd pairs are built ONCE and
        // used for both the full-resolution store and the pooled one (relu and the bf16 rounding are
        // monotonic and every value is >= 0 after the relu, so the packed int16 max of the stored bits IS
        // the pooled tensor; the epilogue's VALU instructions are paid at the partner wave's MFMA cadence).
#pragma unroll
        for (int n = 0; n < NF; ++n) {
            if (((n / FR) & 1) != 0) continue;  // upper row of each pair
            uint4 pk[2][2];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int nn = n + r * FR;
                const int y = y0 + wp * ROWS_W + nn / FR;
                const int x = x0 + (nn % FR) * 16 + l15;
                const bool ok = (y < aH) && (x < aW);
                char* o = out_img + (size_t)(y * aW + x) * 64;
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    uint4 v = make_uint4(pack2_pk<T>(acc[2 * g][nn][0], acc[2 * g][nn][1]),
                                         pack2_pk<T>(acc[2 * g][nn][2], acc[2 * g][nn][3]),
                                         pack2_pk<T>(acc[2 * g + 1][nn][0], acc[2 * g + 1][nn][1]),
                                         pack2_pk<T>(acc[2 * g + 1][nn][2], acc[2 * g + 1][nn][3]));
                    if (a.relu) v = make_uint4(relu_pk_bf16(v.x), relu_pk_bf16(v.y), relu_pk_bf16(v.z), relu_pk_bf16(v.w));
                    pk[r][g] = v;
                    if (ok && out_img) *reinterpret_cast<uint4*>(o + g * plane_stride) = v;
                }
            }
            const int y = y0 + wp * ROWS_W + n / FR;
            const int x = x0 + (n % FR) * 16 + l15;
            const int py = y >> 1, px = x >> 1;
            const bool okp = (py < pH) && (px < pW) && ((l15 & 1) == 0);
            char* o = pool_img + (size_t)(min(py, pH - 1) * pW + min(px, pW - 1)) * 64;
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                const uint4 t = pk[0][g], u = pk[1][g];
                const unsigned c0 = pk_max_i16(t.x, u.x), c1 = pk_max_i16(t.y, u.y);
                const unsigned c2 = pk_max_i16(t.z, u.z), c3 = pk_max_i16(t.w, u.w);
                const uint4 m = make_uint4(pk_max_i16(c0, dpp_swap_pairs(c0)), pk_max_i16(c1, dpp_swap_pairs(c1)),
                                           pk_max_i16(c2, dpp_swap_pairs(c2)), pk_max_i16(c3, dpp_swap_pairs(c3)));
                if (okp) *reinterpret_cast<uint4*>(o + g * pplane_stride) = m;
            }
        }
        return;
    }
#pragma unroll
    for (int n = 0; n < NF; ++n) {
        const int y = y0 + wp * ROWS_W + n / FR;
        const int x = x0 + (n % FR) * 16 + l15;
        const bool ok = (y < aH) && (x < aW);
        if (ok && out_img) {
            char* o = out_img + (size_t)(y * aW + x) * 64;
            if constexpr (PERM) {
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    uint4 pk = make_uint4(pack2<T>(acc[2 * g][n][0], acc[2 * g][n][1]),
                                          pack2<T>(acc[2 * g][n][2], acc[2 * g][n][3]),
                                          pack2<T>(acc[2 * g + 1][n][0], acc[2 * g + 1][n][1]),
                                          pack2<T>(acc[2 * g + 1][n][2], acc[2 * g + 1][n][3]));
                    if (a.relu) pk = make_uint4(relu_pk_bf16(pk.x), relu_pk_bf16(pk.y), relu_pk_bf16(pk.z), relu_pk_bf16(pk.w));
                    *reinterpret_cast<uint4*>(o + g * plane_stride) = pk;
                }
            } else {
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    float4 v = make_float4(acc[m][n][0], acc[m][n][1], acc[m][n][2], acc[m][n][3]);
                    if (a.relu) v = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
                    *reinterpret_cast<float4*>(o + m * plane_stride) = v;
                }
            }
        }
    }
    if (EPI == EPI_POOL) {
        // MaxPool2d(2) of this conv's output (unet.py:28), fused here so the consumer conv reads a
        // ready tensor by LDS-DMA: tile origins are even, a wave owns whole row pairs (fragments n
        // and n+FR) and the column partner is the neighbouring lane (l15 ^ 1).
        // relu and the bf16 rounding are monotonic, so max-then-relu-then-round of the raw sums
        // equals pooling the stored tensor.
#pragma unroll
        for (int n = 0; n < NF; ++n) {
            if (((n / FR) & 1) != 0) continue;  // upper row of each pair only
            const int y = y0 + wp * ROWS_W + n / FR;
            const int x = x0 + (n % FR) * 16 + l15;
            const int py = y >> 1, px = x >> 1;
            const bool okp = (py < pH) && (px < pW) && ((l15 & 1) == 0);
            char* o = pool_img + (size_t)(min(py, pH - 1) * pW + min(px, pW - 1)) * 64;
            if constexpr (!PERM) {
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    float r[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float cm = fmaxf(acc[m][n][j], acc[m][n + FR][j]);
                        r[j] = fmaxf(cm, __uint_as_float(dpp_swap_pairs(__float_as_uint(cm))));
                        if (a.relu) r[j] = fmaxf(r[j], 0.f);
                    }
                    if (okp) *reinterpret_cast<float4*>(o + m * pplane_stride) = make_float4(r[0], r[1], r[2], r[3]);
                }
            } else {
                // Packed int16 max on the rounded bf16 pairs.  Among non-negative patterns it is the
                // float max; a negative pattern (sign bit) loses against every non-negative one, so
                // the result is the true maximum whenever that is >= 0 and SOME negative value
                // otherwise -- which the final relu turns into 0 either way: relu(max) exactly.
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    unsigned r[4];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int m = 2 * g + h;
                        const unsigned a0 = pk_max_i16(pack2_pk<T>(acc[m][n][0], acc[m][n][1]),
                                                       pack2_pk<T>(acc[m][n + FR][0], acc[m][n + FR][1]));
                        const unsigned a1 = pk_max_i16(pack2_pk<T>(acc[m][n][2], acc[m][n][3]),
                                                       pack2_pk<T>(acc[m][n + FR][2], acc[m][n + FR][3]));
                        r[2 * h] = pk_max_i16(a0, dpp_swap_pairs(a0));
                        r[2 * h + 1] = pk_max_i16(a1, dpp_swap_pairs(a1));
                        if (a.relu) { r[2 * h] = relu_pk_bf16(r[2 * h]); r[2 * h + 1] = relu_pk_bf16(r[2 * h + 1]); }
                    }
                    if (okp) *reinterpret_cast<uint4*>(o + g * pplane_stride) = make_uint4(r[0], r[1], r[2], r[3]);
                }
            }
        }
    }
}

}  // namespace fiunet
