/*
 * fiunet.h -- C ABI of the MI355X-native UNet frame-pair forward (libfiunet_hip.so).
 *
 * The reference (daultanigaurav/AI-BASED-FRAME-INTERPOLATION) has no FFI / plugin layer: its
 * boundary for this path is a Python class plus a state-dict.  Each entry
 * point below therefore replaces a piece of that Python surface, cited as reference file:line.
 * Plain pointers and sizes only; no torch types; every function returns an int status
 * (0 == FIUNET_OK) and never throws across the ABI.  Device pointers are HIP device memory
 * of the context's device; `stream` is a hipStream_t passed as void* (NULL = default stream).
 * All launches are asynchronous on that stream; one in-flight call per ctx+stream.
 *
 * See INTEGRATION.md for the reference-side binding (a ctypes stub in model/unet.py).
 */
#ifndef FIUNET_H
#define FIUNET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FIUNET_ABI_VERSION 8   /* 4: fiunet_prepare_precision; fiunet_debug_read_activation takes the capacity of dst; 5: fiunet_forward_u8_strided;
                                  6: YUV 4:2:0 colour video (fiunet_yuv420_to_rgb_u8, fiunet_rgb_to_yuv420_u8, fiunet_forward_yuv420);
                                  7: 10-bit video (fiunet_forward_p10, fiunet_forward_yuv420p10 and their pieces; FIUNET_YUV_BT2020);
                                  8: precision FIUNET_FP16; v8 also: scene-cut entry points (fiunet_pair_sad_u8,
                                     fiunet_pair_sad_p10, fiunet_scene_cuts, fiunet_hold_cut_frames) and frame-rate conversion
                                     (fiunet_retime_u8, fiunet_retime_p10), backwards-compatible; v8 also, added the same
                                     way: NV12 / P010 decoder surfaces (fiunet_surface_layout, fiunet_nv12_to_rgb_u8,
                                     fiunet_rgb_to_nv12_u8, fiunet_forward_nv12, fiunet_p010_to_rgb_p10,
                                     fiunet_rgb_p10_to_p010, fiunet_forward_p010 and the two workspace queries); v8 also, added
                                     the same way: packed RGB frames (fiunet_packed_format, fiunet_packed_layout,
                                     fiunet_packed_to_rgb_u8, fiunet_rgb_to_packed_u8, fiunet_forward_rgb_packed and its
                                     workspace query); v8 also, added the same way: PSNR / SSIM on strided 8- and 10-bit
                                     planes (fiunet_plane_psnr, fiunet_plane_ssim and their workspace query); v8 also, added
                                     the same way: Farneback flow and flow-compensated warps (fiunet_flow_workspace_bytes,
                                     fiunet_farneback_flow, fiunet_flow_warp, fiunet_flow_mode); v8 also, added the same
                                     way: the plane metrics on interleaved samples (fiunet_interleaved_psnr,
                                     fiunet_stepped_ssim); v8 also, added the same way: repeated frames in video
                                     (fiunet_pair_peak_u8, fiunet_pair_peak_p10, fiunet_retime_table_u8,
                                     fiunet_retime_table_p10); v8 also, added the same way: resizing frame planes
                                     (fiunet_resize_plane, fiunet_resize_planes_u8, fiunet_resize_planes_p10); v8 also: the
                                     `reserved` member of fiunet_resize_plane, which had to be 0, is `filter`
                                     (FIUNET_RESIZE_LINEAR = 0, FIUNET_RESIZE_AREA); no entry point is added; v8 also,
                                     added the same way: 10-bit 4:2:2 wire packings (fiunet_packing10,
                                     fiunet_unpack_422p10, fiunet_pack_422p10); v8 also, added the same way:
                                     motion-compensated resampling (fiunet_warp_entry, fiunet_warp_table_u8,
                                     fiunet_warp_table_p10); v8 also, added the same way: motion-guided chroma
                                     (fiunet_chroma_pick_u8, fiunet_chroma_pick_p10, fiunet_chroma_fill_u8,
                                     fiunet_chroma_fill_p10); v8 also, added the same way: deinterlacing
                                     (fiunet_deinterlace_u8, fiunet_deinterlace_p10); v8 also, added the same way: inverse
                                     telecine (fiunet_weave_entry, fiunet_field_match_u8, fiunet_field_match_p10,
                                     fiunet_field_weave_u8, fiunet_field_weave_p10); v8 also, added the same way: a
                                     synthesized shutter for lower frame rates (fiunet_shutter_u8, fiunet_shutter_p10) */

enum fiunet_status {
    FIUNET_OK = 0,
    FIUNET_ERR_INVALID_ARG = 1,   /* bad pointer / size (the reference raises RuntimeError) */
    FIUNET_ERR_BAD_SHAPE = 2,     /* H or W < 16 (reference: max-pool raises) */
    FIUNET_ERR_MISSING_WEIGHT = 3,/* a state-dict tensor is absent or has the wrong numel */
    FIUNET_ERR_NOT_LOADED = 4,    /* forward before load_weights */
    FIUNET_ERR_WORKSPACE = 5,     /* workspace too small */
    FIUNET_ERR_HIP = 6,           /* a HIP runtime call failed; see fiunet_last_error_string */
    FIUNET_ERR_UNSUPPORTED = 7    /* a value outside what the kernels cover (fiunet_ssim_gauss_f32: even or > 31 window;
                                     read-back of an upsampled half that is never stored) */
};

/* Arithmetic type of the conv path.  FP32: fp32 storage, exact-fp32 MFMA (v_mfma_f32_16x16x4_f32).
 * BF16 / FP16: bf16 / fp16 activations/weights in HBM, v_mfma_f32_16x16x32_bf16 / _f16 with fp32 accumulation; the
 * first (Cin=2) conv and the final 1x1 conv stay fp32 arithmetic in every mode. */
enum fiunet_precision {
    FIUNET_FP32 = 0,   /* exact fp32: v_mfma_f32_16x16x4_f32 (the reference's own arithmetic) */
    FIUNET_BF16 = 1,   /* bf16 storage and MFMA operands, fp32 accumulation */
    FIUNET_BF16X2 = 2, /* the fp32 CONTRACT (|d| <= 1e-3) on the bf16 pipe - every activation and weight is two bf16
                          pieces (hi + lo, 16 significant bits; activations [hi planes | lo planes], 4 B per element), a
                          product is wh*xh + wl*xh + wh*xl with fp32 accumulation (~1e-5 relative end to end); fp32 frames
                          in, fp32 logits out, exact-fp32 stem and head.  Needs fiunet_prepare_precision(ctx, FIUNET_BF16X2)
                          once after fiunet_load_weights.  Both decoders; FIUNET_OPT_KEEP_ALL + read-back work, the other
                          A/B options (UNFUSED, GATHER_UPSAMPLE) are ignored in this mode */
    FIUNET_FP16 = 3    /* IEEE fp16 storage and MFMA operands (v_mfma_f32_16x16x32_f16, bf16's shape and rate), fp32
                          accumulation: bf16's kernels, tiles and launch plan with 11 significant bits instead of 8.  Every
                          rounding to fp16 is to nearest even and saturates at +-65504; the weights are rounded to nearest
                          (no error feedback) and the stem has no dither - FIUNET_OPT_RNE_WEIGHTS and FIUNET_OPT_NO_DITHER are
                          bf16-only and change nothing here.  The stems keep bf16's arithmetic (split-bf16 MFMAs / exact fp32)
                          and round their output to fp16; the 1x1 head is fp32.  UNFUSED, KEEP_ALL and GATHER_UPSAMPLE work as
                          in BF16.  Needs fiunet_prepare_precision(ctx, FIUNET_FP16) once after fiunet_load_weights */
};

/* Bit flags for fiunet_set_options. */
enum fiunet_option {
    FIUNET_OPT_UNFUSED = 1, /* ablation: run max-pool, upsample+pad+concat and the 1x1 head as
                               separate kernels instead of fusing them into the consumer conv */
    FIUNET_OPT_KEEP_ALL = 2,/* also store the last 64-ch activation (tap 17) that the fused 1x1
                               head otherwise keeps in registers; for fiunet_debug_read_activation */
    FIUNET_OPT_RNE_WEIGHTS = 32, /* A/B runs: round the bf16 conv weights to nearest instead of with the per-filter
                               error feedback (fiunet.hip, f32_to_bf16_feedback).  Read by fiunet_load_weights: set it
                               BEFORE loading */
    FIUNET_OPT_NO_DITHER = 64, /* A/B runs: switch off the ordered input dither of the bf16 stem (+-2^-9 on the
                               frames, +d on frame 1 / -d on frame 2, an 8x8 Bayer pattern of the global pixel
                               position: it decorrelates the bf16 rounding of values the network carries through
                               its full-resolution skip from the image content; conv3x3_mfma.hip.h, stem_dither) */
    FIUNET_OPT_GATHER_UPSAMPLE = 16 /* A/B runs and tests: always interpolate the upsampled half of a concat
                               input inside the conv's gather; by default the bf16 convs with >= 2 cout tiles
                               on >= 64k pixels read it from a tensor written once by upsample_kernel; same bits */
};

typedef struct fiunet_ctx fiunet_ctx;

/* Replaces FrameInterpolationUNet.__init__ / UNet.__init__ (model/unet.py:99-103, :66-82).
 * frame_channels: 1 = grayscale (the reference's 2->1 network), 3 = RGB (6->3, README variant).
 * bilinear: 1 = bilinear-upsample decoder, what every reference caller constructs (model/inference.py:77);
 * 0 = the constructor's default (model/unet.py:66,99): ConvTranspose2d(C, C/2, 2, 2) decoder (unet.py:42-44), widths
 * 64-128-256-512-1024, 118-tensor state-dict with `unet.up{k}.up.weight/bias`. */
int fiunet_create(fiunet_ctx** out_ctx, int device_id, int frame_channels, int bilinear);

/* Replaces nn.Module teardown (Python GC). */
int fiunet_destroy(fiunet_ctx* ctx);

int fiunet_set_options(fiunet_ctx* ctx, unsigned flags);

/* Replaces model.load_state_dict(...) + .to(device) + .eval() (model/inference.py:83-97).
 * `names[i]` are reference state-dict keys ("unet.inc.double_conv.0.weight", ...),
 * `host_ptrs[i]` contiguous fp32 host arrays, `numels[i]` their element counts.  The
 * `num_batches_tracked` counters may be omitted or passed (ignored).  The library folds the
 * eval-mode BatchNorm into a per-channel scale/shift, repacks OIHW weights into its kernel
 * layout for both precisions and owns the device copies. */
int fiunet_load_weights(fiunet_ctx* ctx, int n, const char* const* names,
                        const float* const* host_ptrs, const int64_t* numels);

/* fiunet_load_weights for tensors that are already in the memory of the context's GPU (v8, added without a version
 * bump): the same keys, the same sizes and the same FIUNET_ERR_MISSING_WEIGHT messages, `device_ptrs[i]` contiguous fp32
 * device arrays.  HIP kernels fold, repack and round there and leave, bit for bit, the buffers fiunet_load_weights
 * leaves (the rounding mode of FIUNET_OPT_RNE_WEIGHTS is read at this call, as there).  Every key is checked before
 * anything changes: a call that fails on a key leaves the weights loaded before it in place and usable.  The first
 * load of a context allocates; a later one (after either entry point) packs into the same buffers - no allocation, no
 * free, no host synchronisation, the kernels asynchronous on `stream`, which is also where they read `device_ptrs`:
 * keep those alive, and order forwards on other streams, behind it.  The copies of fiunet_prepare_precision are stale
 * afterwards, as after fiunet_load_weights: call it again (it waits for this load on the device, not on the host).
 * The one exception to "bit for bit": a NaN that the fold itself creates - an infinite weight in a channel whose folded
 * scale is zero - has the sign bit set from the host (x86) and clear from the GPU.  NaN and infinite weights with a
 * non-zero scale come out identical. */
int fiunet_load_weights_device(fiunet_ctx* ctx, int n, const char* const* names,
                               const float* const* device_ptrs, const int64_t* numels, void* stream);

/* Builds the weight copies a precision needs beyond what fiunet_load_weights made (FP32, BF16: nothing; BF16X2: the
 * two-piece [wh | wl] copies, ~69 MB, packed on the device from the fp32 copy; FP16: the fp16 copies, ~35 MB, rounded
 * to nearest even on the device from the fp32 copy).  Call it after fiunet_load_weights and
 * before the first forward in that precision (a forward without it returns FIUNET_ERR_NOT_LOADED); idempotent;
 * allocates and synchronises - so not under stream capture.  The reference has no counterpart: its one precision is
 * whatever dtype the module's tensors have (model/inference.py:96). */
int fiunet_prepare_precision(fiunet_ctx* ctx, int precision);

/* Bytes of device scratch fiunet_forward needs for a [B,*,H,W] batch; 0 on bad arguments and for a shape no forward
 * takes (fiunet_last_error_string says which: H or W below 16, 2^26 pixels or more, or a materialised upsample whose
 * launch grid would pass 65535 - bf16x2 frames taller than 524 280 rows, batches of 4096 and more): the shape is refused
 * here, where the plan is made, and a forward of it launches nothing.
 * Activations whose lifetimes do not overlap share bytes (the reference, under no_grad, frees every
 * non-skip tensor as it goes: model/unet.py:84-95), so the figure depends on the options in force
 * (FIUNET_OPT_KEEP_ALL pins all 18 activations, FIUNET_OPT_UNFUSED adds the concat scratch): query it
 * AFTER fiunet_set_options.  B=8 1080x1920: 6.4 GB bf16 / 12.8 GB fp32. */
size_t fiunet_workspace_bytes(const fiunet_ctx* ctx, int B, int H, int W, int precision);

/* Smallest batch B (1..64; 65 = none) at which NO layer of a forward of H x W frames cuts its K loop over several
 * workgroups (see "Reproducibility" below): batches of at least that many pairs give every pair the same bits whatever
 * the batch.  1 from 1080p up; at 720p 3 in fp32 and 2 in bf16 / bf16x2 (round 6 rule; 5 until round 5); > 8 for the
 * reference's own 256x256.  The value holds for the context's current options, default tile choice included.  Needs loaded weights (it walks the
 * architecture); 0 on bad arguments.  Used by the video loops to pad a ragged last chunk no further than necessary.
 * The reference has no counterpart (aten's conv results do depend on the batch in the last bit). */
int fiunet_min_unsplit_batch(const fiunet_ctx* ctx, int H, int W, int precision);

/* Replaces FrameInterpolationUNet.forward(frame1, frame2) in eval mode
 * (model/unet.py:105-112 -> :84-95), as called by interpolate_frames (model/inference.py:120).
 * frame1, frame2: device fp32 [B, frame_channels, H, W] contiguous (NCHW);
 * out: device fp32 [B, frame_channels, H, W]; raw logits, no activation.
 * workspace: device scratch of at least fiunet_workspace_bytes(...), 256-B aligned.
 * Reproducibility: a call is deterministic (no atomics; fixed summation order).  For frames of >= 1080p the
 * result of a pair does not depend on the batch it is part of or on its position (bit for bit); for smaller
 * frames that holds among batches of at least fiunet_min_unsplit_batch(ctx, H, W, precision) pairs (2 at 720p, bf16).
 * Below that, layers with fewer workgroups than the chip has CUs cut their K loop over several workgroups, and
 * how many depends on B, so the fp32 summation order of a pair - hence its last bit - may differ between batch
 * sizes (1.8e-5 in fp32 on O(1) outputs, bf16 ulp flips; the same holds for a short band of
 * fiunet_forward_strip against the whole frame).  Callers that need a sequence's result to be independent of how
 * it was batched should pad a ragged last batch up to that size, or to the full batch where even a full batch
 * splits (ai_based_frame_interpolation_amd/inference.py does). */
int fiunet_forward(fiunet_ctx* ctx, const float* frame1, const float* frame2, float* out, int B,
                   int H, int W, int precision, void* workspace, size_t workspace_bytes,
                   void* stream);

/* Spatial tiling (2160x3840 pairs cut into horizontal strips, one per
 * GPU).  The reference has no counterpart: it is the same forward (model/unet.py:84-95) evaluated on
 * the band of rows [y_origin, y_origin + H) of an image of H_image rows.  frame1, frame2, out are that
 * band only ([B, C, H, W] contiguous).  The align_corners=True upsampling (unet.py:40) and the F.pad
 * offsets (unet.py:49-53) are evaluated in whole-image coordinates, so every output row whose
 * receptive field (+-109 rows) lies inside the band - or is cut only by a true image border - equals
 * the un-tiled result; rows nearer to a cut edge see zero padding there and must be discarded by the
 * caller (use a halo of >= 112 rows).  y_origin must be a multiple of 16 (four 2x2 max-pools) and H a
 * multiple of 16 unless the band ends the image.  fiunet_forward(..., H, ...) is the band
 * y_origin = 0, H_image = H.  Workspace: fiunet_workspace_bytes(ctx, B, H, W, precision). */
int fiunet_forward_strip(fiunet_ctx* ctx, const float* frame1, const float* frame2, float* out, int B,
                         int H, int W, int y_origin, int H_image, int precision, void* workspace,
                         size_t workspace_bytes, void* stream);

/* Video-path variant: uint8 frames in, uint8 interpolated frame out, with the reference's
 * pre/post-processing on device: x/255*2-1 (model/inference.py:31-35) where the frames are read and
 * trunc(clamp((y+1)/2,0,1)*255) (model/inference.py:54-61) where the output is written, bit for bit the
 * values fiunet_preprocess_u8 -> fiunet_forward -> fiunet_postprocess_u8 give.  frame1/2, out: device uint8
 * [B, frame_channels, H, W].  Where the stem conv is evaluated inside the next conv's gather (bf16, gray)
 * it reads the uint8 frames itself, and every fused 1x1 head writes uint8 itself: one launch chain, no
 * fp32 frame buffers; the other configurations (fp32 / RGB stem kernel, FIUNET_OPT_UNFUSED, FIUNET_OPT_KEEP_ALL)
 * run the two elementwise kernels around the forward on up to three fp32 buffers.  Workspace:
 * fiunet_workspace_bytes_u8 (query it after fiunet_set_options). */
size_t fiunet_workspace_bytes_u8(const fiunet_ctx* ctx, int B, int H, int W, int precision);
int fiunet_forward_u8(fiunet_ctx* ctx, const uint8_t* frame1, const uint8_t* frame2, uint8_t* out,
                      int B, int H, int W, int precision, void* workspace, size_t workspace_bytes,
                      void* stream);
/* The same with the B output images `out_image_stride` BYTES apart (0 = contiguous; >= frame_channels * H * W): the
 * factor-2 video loop (the phantom `interpolate_video` of /root/reference/main.py:118-129) hands
 * over every second frame of its interleaved result F0 M0 F1 M1 ..., so the fused head writes each interpolated frame
 * where it belongs - no temporary, no strided copy afterwards.  Everything else as fiunet_forward_u8. */
int fiunet_forward_u8_strided(fiunet_ctx* ctx, const uint8_t* frame1, const uint8_t* frame2, uint8_t* out,
                              size_t out_image_stride, int B, int H, int W, int precision, void* workspace,
                              size_t workspace_bytes, void* stream);

/* Colour video for the RGB (frame_channels == 3) network.  The reference has no colour path; these entry points link
 * the container a decoder gives (YUV 4:2:0, `ffmpeg -i in.mp4 -pix_fmt yuv420p in.y4m`) to the planar RGB network.
 * A frame is packed I420, exactly a Y4M frame payload: the Y plane H x W, then U, then V, each ceil(H/2) x ceil(W/2)
 * bytes (fiunet frame size F = H*W + 2*ceil(H/2)*ceil(W/2)).  The conversion is defined in integer arithmetic
 * (csrc/colour.hip.h, DESIGN.md "Colour video"), so it is the same bits on every device.  `colour` is a set of flags;
 * 0 = jpeg siting (also Y4M `420` / no tag), BT.601, limited range; any other bit is FIUNET_ERR_INVALID_ARG. */
enum fiunet_colour {
    FIUNET_YUV_MPEG2 = 1,      /* chroma siting 420mpeg2: co-sited with the even luma column, centred vertically
                                  (default: 420jpeg, centred in its 2x2 luma block) */
    FIUNET_YUV_BT709 = 2,      /* matrix BT.709 (Kr 0.2126, Kb 0.0722); default BT.601 (Kr 0.299, Kb 0.114) */
    FIUNET_YUV_FULL_RANGE = 4, /* Y 0-255, C = 128 + 255 E'P; default limited: Y 16-235, C 16-240
                                  (10-bit: Y 0-1023, C = 512 + 1023 E'P; limited Y 64-940, C 64-960) */
    FIUNET_YUV_BT2020 = 8      /* matrix BT.2020 non-constant luminance (Kr 0.2627, Kb 0.0593): the 10-bit entry points
                                  only (the 8-bit ones reject it: BT.2020 defines 10- and 12-bit coding); together with
                                  FIUNET_YUV_BT709 it is FIUNET_ERR_INVALID_ARG */
};

/* Packed I420 frames (`in_frame_stride` bytes apart, 0 = F) -> planar RGB uint8 [B, 3, H, W] (the layout
 * fiunet_forward_u8 takes for frame_channels == 3).  Device pointers; any H, W >= 1 (odd sizes included).
 * Asynchronous on `stream`; no allocation, no synchronisation. */
int fiunet_yuv420_to_rgb_u8(const uint8_t* in, size_t in_frame_stride, uint8_t* out, int B, int H, int W,
                            unsigned colour, void* stream);
/* The inverse: planar RGB uint8 [B, 3, H, W] -> packed I420 frames `out_frame_stride` bytes apart (0 = F; bytes
 * between frames are left untouched). */
int fiunet_rgb_to_yuv420_u8(const uint8_t* in, uint8_t* out, size_t out_frame_stride, int B, int H, int W,
                            unsigned colour, void* stream);
/* Workspace of fiunet_forward_yuv420: fiunet_workspace_bytes_u8 plus three planar RGB batches; 0 on bad arguments
 * (query it after fiunet_set_options). */
size_t fiunet_workspace_bytes_yuv420(const fiunet_ctx* ctx, int B, int H, int W, int precision);
/* The video-path forward on packed I420 frames: frame1, frame2 are B frames of F bytes each, contiguous; the B
 * interpolated frames go to `out`, `out_frame_stride` bytes apart (0 = F; the video loop hands over every second frame
 * of its interleaved result).  Three steps in the caller's workspace: fiunet_yuv420_to_rgb_u8 of both inputs,
 * fiunet_forward_u8_strided into a planar RGB buffer, fiunet_rgb_to_yuv420_u8 into `out` - bit for bit the chain of
 * those public calls.  FIUNET_ERR_UNSUPPORTED on a context with frame_channels != 3.  Neither allocates nor
 * synchronises: it captures into a graph as fiunet_forward_u8 does.  This and every fiunet_forward_<format> below make
 * every refusal before their first launch, FIUNET_ERR_NOT_LOADED on a context without weights included. */
int fiunet_forward_yuv420(fiunet_ctx* ctx, const uint8_t* frame1, const uint8_t* frame2, uint8_t* out,
                          size_t out_frame_stride, int B, int H, int W, unsigned colour, int precision,
                          void* workspace, size_t workspace_bytes, void* stream);

/* 10-bit video (ABI v7).  The reference has no counterpart.  A sample is a 10-bit code in a uint16 word (what a
 * `C420p10` / `Cmono10` Y4M payload holds, little-endian); any sample above 1023 is read as 1023.  The network sees
 * pre10(x) = x / 1023 * 2 - 1 (the IEEE fp32 quotient) and its output is written as post10(t) =
 * trunc(clamp((t + 1) / 2, 0, 1) * 1023): the u8 pre/post-processing with 1023 in place of 255.
 * Device pointers; asynchronous on `stream`; no allocation, no synchronisation. */
int fiunet_preprocess_p10(const uint16_t* in, float* out, size_t n, void* stream);
int fiunet_postprocess_p10(const float* in, uint16_t* out, size_t n, void* stream);
/* Workspace of fiunet_forward_p10: fiunet_workspace_bytes plus three fp32 frame batches; 0 on bad arguments (query it
 * after fiunet_set_options). */
size_t fiunet_workspace_bytes_p10(const fiunet_ctx* ctx, int B, int H, int W, int precision);
/* The forward on 10-bit frames, both networks: frame1, frame2 device uint16 [B, frame_channels, H, W]; the B output
 * images go to `out`, `out_image_stride` SAMPLES apart (0 = contiguous; >= frame_channels * H * W).  pre10 of both
 * inputs into fp32 staging, fiunet_forward, post10 into `out` - bit for bit fiunet_preprocess_p10 -> fiunet_forward
 * -> fiunet_postprocess_p10.  Accuracy: fp32 and FIUNET_BF16X2 within 1 code of the fp32 oracle; FIUNET_BF16 about
 * 5 codes (8 significant bits; its stem dither is 2 ten-bit codes peak to peak); FIUNET_FP16 within 1 code at nearly
 * bf16's speed: use FIUNET_FP16 (or FIUNET_BF16X2) for 10-bit video. */
int fiunet_forward_p10(fiunet_ctx* ctx, const uint16_t* frame1, const uint16_t* frame2, uint16_t* out,
                       size_t out_image_stride, int B, int H, int W, int precision, void* workspace,
                       size_t workspace_bytes, void* stream);
/* 10-bit YUV 4:2:0 <-> planar RGB: the 8-bit conversions above on 10-bit samples (a frame is F = H*W +
 * 2*ceil(H/2)*ceil(W/2) SAMPLES, a C420p10 Y4M payload; every frame stride is counted in SAMPLES, 0 = F).  Limited
 * range Y = 64 + 876 E'Y, C = 512 + 896 E'P; full range Y = 1023 E'Y, C = 512 + 1023 E'P; results clamped to
 * [0, 1023].  `colour` as for the 8-bit calls plus FIUNET_YUV_BT2020. */
int fiunet_yuv420p10_to_rgb_p10(const uint16_t* in, size_t in_frame_stride, uint16_t* out, int B, int H, int W,
                                unsigned colour, void* stream);
int fiunet_rgb_p10_to_yuv420p10(const uint16_t* in, uint16_t* out, size_t out_frame_stride, int B, int H, int W,
                                unsigned colour, void* stream);
/* Workspace of fiunet_forward_yuv420p10: fiunet_workspace_bytes_p10 plus three planar RGB uint16 batches. */
size_t fiunet_workspace_bytes_yuv420p10(const fiunet_ctx* ctx, int B, int H, int W, int precision);
/* fiunet_forward_yuv420 on 10-bit frames: B packed 4:2:0 frames of F samples each, contiguous, in; the B interpolated
 * frames to `out`, `out_frame_stride` SAMPLES apart (0 = F).  Bit for bit fiunet_yuv420p10_to_rgb_p10 (both inputs) ->
 * fiunet_forward_p10 -> fiunet_rgb_p10_to_yuv420p10.  FIUNET_ERR_UNSUPPORTED on a context with frame_channels != 3.
 * Neither allocates nor synchronises. */
int fiunet_forward_yuv420p10(fiunet_ctx* ctx, const uint16_t* frame1, const uint16_t* frame2, uint16_t* out,
                             size_t out_frame_stride, int B, int H, int W, unsigned colour, int precision,
                             void* workspace, size_t workspace_bytes, void* stream);

/* Semi-planar decoder surfaces (ABI v8, added without a version bump: nothing existing changed): NV12
 * at 8 bits and P010 at 10, what a hardware decoder (VCN behind rocDecode, ffmpeg's hwaccel `nv12` / `p010le`) leaves in
 * device memory and what hardware encoders take.  The arithmetic is exactly that of the 4:2:0 entry points above
 * (csrc/colour.hip.h: siting, matrix, range, rounding and clamps); only where a sample lives differs.
 * Layout, every quantity in SAMPLES (bytes at 8 bits, 16-bit words at 10), with Hc = ceil(H/2), Wc = ceil(W/2): a frame
 * is H luma rows `luma_pitch` apart; from `chroma_offset` samples after the frame's base come Hc chroma rows
 * `chroma_pitch` apart, each holding Wc pairs U0 V0 U1 V1 ...; frames are `frame_stride` apart.  The tight layout is
 * luma_pitch = W, chroma_offset = H*W, chroma_pitch = 2*Wc, frame_stride = H*W + 2*Hc*Wc = F, the size of an I420
 * frame.  A field that is 0 takes its tight value (a pitched surface names every field that differs); a NULL layout is
 * the tight one.  FIUNET_ERR_INVALID_ARG, before any launch: luma_pitch < W, chroma_pitch < 2*Wc, chroma_offset <
 * (H-1)*luma_pitch + W, or frame_stride < chroma_offset + (Hc-1)*chroma_pitch + 2*Wc (it does not cover the chroma
 * plane).  Samples outside the W / 2*Wc used columns and between the planes are never read and never written.
 * P010: a word is code << 6; read as word >> 6, the low six bits ignored whatever they hold; written with them zero.
 * For a rocDecode / VCN surface: luma_pitch = chroma_pitch = the surface pitch (in samples), chroma_offset = pitch x
 * the aligned surface height, frame_stride = the distance between surfaces (or 0 with B = 1 and a tight one). */
typedef struct fiunet_surface_layout {
    size_t luma_pitch, chroma_offset, chroma_pitch, frame_stride;
} fiunet_surface_layout;
/* NV12 surfaces -> planar RGB uint8 [B, 3, H, W], and back: fiunet_yuv420_to_rgb_u8 / fiunet_rgb_to_yuv420_u8 on the
 * layout above.  With W, every layout value and the bases multiples of 4 samples, a thread's two chroma pairs are one
 * 4-sample access.  Device pointers; any H, W >= 1; asynchronous on `stream`; no allocation, no synchronisation. */
int fiunet_nv12_to_rgb_u8(const uint8_t* in, const fiunet_surface_layout* in_layout, uint8_t* out, int B, int H, int W,
                          unsigned colour, void* stream);
int fiunet_rgb_to_nv12_u8(const uint8_t* in, uint8_t* out, const fiunet_surface_layout* out_layout, int B, int H, int W,
                          unsigned colour, void* stream);
/* Workspace of fiunet_forward_nv12: that of fiunet_forward_yuv420. */
size_t fiunet_workspace_bytes_nv12(const fiunet_ctx* ctx, int B, int H, int W, int precision);
/* fiunet_forward_yuv420 on NV12 surfaces (layout above): frame1 and frame2 in `in_layout`, the B interpolated frames to
 * `out` in `out_layout`.  Bit for bit fiunet_nv12_to_rgb_u8 (both inputs) -> fiunet_forward_u8_strided ->
 * fiunet_rgb_to_nv12_u8; both layouts are checked before the first launch.  FIUNET_ERR_UNSUPPORTED on a context with
 * frame_channels != 3.  Neither allocates nor synchronises. */
int fiunet_forward_nv12(fiunet_ctx* ctx, const uint8_t* frame1, const uint8_t* frame2,
                        const fiunet_surface_layout* in_layout, uint8_t* out, const fiunet_surface_layout* out_layout,
                        int B, int H, int W, unsigned colour, int precision, void* workspace, size_t workspace_bytes,
                        void* stream);
/* The same on P010 surfaces (uint16 words, code << 6) and planar RGB uint16 of 10-bit codes (the layout
 * fiunet_forward_p10 takes): fiunet_yuv420p10_to_rgb_p10 / fiunet_rgb_p10_to_yuv420p10 on the layout above; `colour` as
 * for those.  fiunet_forward_p010 is bit for bit fiunet_p010_to_rgb_p10 (both inputs) -> fiunet_forward_p10 ->
 * fiunet_rgb_p10_to_p010 in the workspace of fiunet_forward_yuv420p10. */
int fiunet_p010_to_rgb_p10(const uint16_t* in, const fiunet_surface_layout* in_layout, uint16_t* out, int B, int H,
                           int W, unsigned colour, void* stream);
int fiunet_rgb_p10_to_p010(const uint16_t* in, uint16_t* out, const fiunet_surface_layout* out_layout, int B, int H,
                           int W, unsigned colour, void* stream);
size_t fiunet_workspace_bytes_p010(const fiunet_ctx* ctx, int B, int H, int W, int precision);
int fiunet_forward_p010(fiunet_ctx* ctx, const uint16_t* frame1, const uint16_t* frame2,
                        const fiunet_surface_layout* in_layout, uint16_t* out, const fiunet_surface_layout* out_layout,
                        int B, int H, int W, unsigned colour, int precision, void* workspace, size_t workspace_bytes,
                        void* stream);

/* YUV 4:2:2 and 4:4:4 frames (ABI v8, added without a version bump: nothing existing changed): what
 * ProRes / DNxHR / XDCAM decode to (yuv422p10le), what SDI and HDMI capture cards deliver (uyvy422 / yuyv422) and what
 * screen and grading sources that stay in YUV hold (yuv444p / yuv444p10le).  The arithmetic extends that of the 4:2:0
 * entry points (csrc/colour.hip.h, csrc/yuv4xx.hip.h): coefficients, ranges, clamps, the Y row and the RGB stage are
 * the same; 4:4:4 chroma is coded per pixel and decoded as it is (the siting flag is ignored); 4:2:2 is the horizontal
 * half of the 4:2:0 rule, chroma row y belonging to luma row y.  The format names are ffmpeg's -pix_fmt names; the
 * sample depth is the entry point's: 8 bits (uint8_t) or 10 (uint16_t words holding the code, little-endian in a file;
 * a word above 1023 reads as 1023). */
enum fiunet_yuv_format {
    FIUNET_YUV_422P = 0,     /* planar: Y plane H x W, then U, then V, each H x ceil(W/2)  (yuv422p, yuv422p10le) */
    FIUNET_YUV_444P = 1,     /* planar: Y, U, V each H x W                                 (yuv444p, yuv444p10le) */
    FIUNET_YUV_UYVY422 = 2,  /* one plane, U0 Y0 V0 Y1 per two pixels; 8 bits only, W even (uyvy422) */
    FIUNET_YUV_YUYV422 = 3   /* one plane, Y0 U0 Y1 V0 per two pixels; 8 bits only, W even (yuyv422) */
};
/* Frames of `format` -> planar RGB [B, 3, H, W] (the layout fiunet_forward_u8 / fiunet_forward_p10 take), and back.
 * Planar formats: frames are tight, `frame_stride` SAMPLES apart (0 = the frame size: 2*H*W for 4:2:2 with W even,
 * H*W + 2*H*ceil(W/2) in general, 3*H*W for 4:4:4); `row_pitch` must be 0; any H, W >= 1.  The two one-plane formats:
 * rows of 2*W bytes `row_pitch` bytes apart (0 = 2*W), frames `frame_stride` bytes apart (0 = H*row_pitch); bytes
 * between 2*W and row_pitch, and between frames, are never read and never written.  With W % 4 == 0 and every base,
 * pitch and stride a multiple of 4 samples a thread's accesses are vector accesses, otherwise per sample.
 * `colour`: as for the 4:2:0 calls of the same depth.  FIUNET_ERR_INVALID_ARG, before any launch: NULL pointers, an
 * unknown format, a one-plane format at 10 bits, FIUNET_YUV_BT2020 at 8 bits, an odd W with a one-plane format, a
 * row_pitch below 2*W (or not 0 with a planar format), a frame_stride that does not cover a frame.  Device pointers;
 * asynchronous on `stream`; no allocation, no synchronisation. */
int fiunet_yuv_to_rgb_u8(const uint8_t* in, int format, size_t row_pitch, size_t frame_stride, uint8_t* out, int B,
                         int H, int W, unsigned colour, void* stream);
int fiunet_rgb_to_yuv_u8(const uint8_t* in, uint8_t* out, int format, size_t row_pitch, size_t frame_stride, int B,
                         int H, int W, unsigned colour, void* stream);
int fiunet_yuv_to_rgb_p10(const uint16_t* in, int format, size_t row_pitch, size_t frame_stride, uint16_t* out, int B,
                          int H, int W, unsigned colour, void* stream);
int fiunet_rgb_p10_to_yuv(const uint16_t* in, uint16_t* out, int format, size_t row_pitch, size_t frame_stride, int B,
                          int H, int W, unsigned colour, void* stream);
/* Workspace of fiunet_forward_yuv (bits 8: that of fiunet_forward_yuv420) and fiunet_forward_yuv_p10 (bits 10: that
 * of fiunet_forward_yuv420p10); 0 on bad arguments. */
size_t fiunet_workspace_bytes_yuv(const fiunet_ctx* ctx, int B, int H, int W, int precision, int bits);
/* The RGB network on frames of `format`: frame1 and frame2 B contiguous frames in (in_row_pitch, in_frame_stride), the
 * B interpolated frames to `out` in (out_row_pitch, out_frame_stride).  Bit for bit fiunet_yuv_to_rgb_u8 (both inputs)
 * -> fiunet_forward_u8_strided -> fiunet_rgb_to_yuv_u8, and at 10 bits fiunet_yuv_to_rgb_p10 -> fiunet_forward_p10 ->
 * fiunet_rgb_p10_to_yuv; every argument is checked before the first launch.  FIUNET_ERR_UNSUPPORTED on a context with
 * frame_channels != 3.  Neither allocates nor synchronises. */
int fiunet_forward_yuv(fiunet_ctx* ctx, const uint8_t* frame1, const uint8_t* frame2, int format, size_t in_row_pitch,
                       size_t in_frame_stride, uint8_t* out, size_t out_row_pitch, size_t out_frame_stride, int B, int H,
                       int W, unsigned colour, int precision, void* workspace, size_t workspace_bytes, void* stream);
int fiunet_forward_yuv_p10(fiunet_ctx* ctx, const uint16_t* frame1, const uint16_t* frame2, int format,
                           size_t in_row_pitch, size_t in_frame_stride, uint16_t* out, size_t out_row_pitch,
                           size_t out_frame_stride, int B, int H, int W, unsigned colour, int precision, void* workspace,
                           size_t workspace_bytes, void* stream);

/* Packed RGB frames (ABI v8, added without a version bump: nothing existing changed): interleaved
 * pixels, what `ffmpeg -f rawvideo -pix_fmt rgb24 | bgr24 | rgba | bgra` pipes and what a screen grab, a render or an
 * image library (BGR rows a line size apart) leaves in memory.  They reach the RGB network with their colour as it is:
 * no chroma subsampling, no colour matrix.  A pixel is 3 or 4 consecutive bytes in the order of the format's name. */
enum fiunet_packed_format {
    FIUNET_PACKED_RGB24 = 0,  /* R G B */
    FIUNET_PACKED_BGR24 = 1,  /* B G R */
    FIUNET_PACKED_RGBA = 2,   /* R G B A */
    FIUNET_PACKED_BGRA = 3    /* B G R A */
};
/* Layout in BYTES, bpp = 3 or 4 by format: a frame is H rows `row_pitch` apart, each W*bpp bytes of pixels; frames are
 * `frame_stride` apart.  A field that is 0 takes its tight value (row_pitch = W*bpp, frame_stride = H*row_pitch); a NULL
 * layout is the tight one.  FIUNET_ERR_INVALID_ARG, before any launch: row_pitch < W*bpp, or frame_stride <
 * (H-1)*row_pitch + W*bpp.  Bytes between W*bpp and row_pitch, and between frames, are never read and never written. */
typedef struct fiunet_packed_layout {
    size_t row_pitch, frame_stride;
} fiunet_packed_layout;
/* Packed frames -> planar RGB uint8 [B, 3, H, W] (the layout fiunet_forward_u8 takes), a move of bytes.  alpha_out: NULL,
 * or (4-byte formats only) where the alpha plane uint8 [B, H, W] goes.  With W, both layout values and every base a
 * multiple of 4 bytes a thread moves its 4 pixels as three dword (bpp 3) or one 16-byte (bpp 4) access and one 4-byte
 * access per plane; otherwise byte by byte.  Device pointers; any H, W >= 1; asynchronous on `stream`; no allocation,
 * no synchronisation.  Errors as for the surface entry points: NULL or an unknown format FIUNET_ERR_INVALID_ARG, a bad
 * shape FIUNET_ERR_BAD_SHAPE. */
int fiunet_packed_to_rgb_u8(const uint8_t* in, const fiunet_packed_layout* in_layout, uint8_t* out_rgb,
                            uint8_t* alpha_out, int B, int H, int W, int format, void* stream);
/* The inverse.  The fourth byte of a 4-byte format: 255 with alpha1 = alpha2 = NULL; a copy of alpha1's alpha byte with
 * alpha1 alone; (a1 + a2 + 1) >> 1 with both.  alpha1 / alpha2 are packed frames of `format`, both in `alpha_layout`
 * (NULL: tight), which need not be `out_layout`.  3-byte formats take no alpha source (FIUNET_ERR_INVALID_ARG), and so
 * does alpha2 without alpha1. */
int fiunet_rgb_to_packed_u8(const uint8_t* in_rgb, uint8_t* out, const fiunet_packed_layout* out_layout,
                            const uint8_t* alpha1, const uint8_t* alpha2, const fiunet_packed_layout* alpha_layout,
                            int B, int H, int W, int format, void* stream);
/* Workspace of fiunet_forward_rgb_packed: that of fiunet_forward_yuv420. */
size_t fiunet_workspace_bytes_rgb_packed(const fiunet_ctx* ctx, int B, int H, int W, int precision);
/* The RGB network on packed frames: frame1 and frame2 in `in_layout`, the B interpolated frames to `out` in
 * `out_layout`.  Bit for bit fiunet_packed_to_rgb_u8 (both inputs) -> fiunet_forward_u8_strided ->
 * fiunet_rgb_to_packed_u8 with frame1 and frame2 as the alpha sources (4-byte formats: the inserted frame's alpha is the
 * rounded average of its neighbours'); both layouts are checked before the first launch.  FIUNET_ERR_UNSUPPORTED on a
 * context with frame_channels != 3.  Neither allocates nor synchronises. */
int fiunet_forward_rgb_packed(fiunet_ctx* ctx, const uint8_t* frame1, const uint8_t* frame2,
                              const fiunet_packed_layout* in_layout, uint8_t* out, const fiunet_packed_layout* out_layout,
                              int B, int H, int W, int format, int precision, void* workspace, size_t workspace_bytes,
                              void* stream);

/* 10-bit 4:2:2 wire packings (ABI v8, added without a version bump: nothing existing changed): v210,
 * y210le and p210le carry the samples of yuv422p10le - FIUNET_YUV_422P at 10 bits: tight frames of uint16 words holding
 * the code, Y H x W, then U, then V, each H x ceil(W/2) - and only the place of the bits differs.  These two entry points
 * move the bits between a packing and that working format; everything else takes the working format.  All wire words
 * are little-endian.
 *   FIUNET_PACK10_V210  one plane, W even.  Group g holds pixels 6g .. 6g+5 in four 32-bit words, each with a low, a
 *                       middle and a high 10-bit field (bits 0-9, 10-19, 20-29): w0 = U0 Y0 V0, w1 = Y1 U1 Y2,
 *                       w2 = V1 Y3 U2, w3 = Y4 V2 Y5 (Uk, Vk: chroma sample 3g + k).  Tight row: 128 * ceil(W / 48) bytes.
 *   FIUNET_PACK10_Y210  one plane, W even.  16-bit words Y0 U0 Y1 V0 per two pixels, each code << 6.  Tight row: 4 W bytes.
 *   FIUNET_PACK10_P210  two planes, any W: a Y plane of H x W words, then H rows of interleaved U V pairs (2 ceil(W/2)
 *                       words), each word code << 6: P010 with chroma of full height.
 * Reading: bits 30-31 of a v210 word and the low six bits of a y210 / p210 word are ignored; v210 fields past column W
 * and row padding are never interpreted.  Writing: the ignored bits are zero, v210 fields past W in the last group are
 * zero, and so are the bytes from the end of the last group to the tight row size, so a tight frame is fully determined;
 * bytes between the tight row and a larger pitch, and between frames, are never read and never written.  A working word
 * above 1023 packs as 1023; no code is clamped to 4..1019.
 * Layouts: v210 / y210le take a fiunet_packed_layout (BYTES, both even; NULL or 0 = tight) and a NULL surface layout;
 * p210le takes a fiunet_surface_layout (SAMPLES; NULL or 0 = tight: chroma_offset H*W, chroma_pitch 2*ceil(W/2),
 * frame_stride H*W + 2*H*ceil(W/2); the chroma plane has H rows) and a NULL packed layout.  out_frame_stride /
 * in_frame_stride: the working frames' distance in samples (0 = tight).  With W % 8 == 0 and every base, pitch, offset
 * and stride a multiple of 16 bytes every access is a 16-, 8- or 4-byte vector with consecutive lanes on consecutive
 * vectors (v210 through LDS), otherwise a thread moves its 24 pixels in 16-bit accesses; both give the same bytes.
 * Device pointers, 2-byte aligned; any H, W >= 1; asynchronous on `stream`; no allocation, no synchronisation.
 * FIUNET_ERR_INVALID_ARG, before any launch: NULL pointers, an unknown packing, an odd W with a one-plane packing, a
 * pitch below the tight row, a stride that does not cover a frame, an odd byte pitch or stride, the layout of the other
 * kind; a bad shape is FIUNET_ERR_BAD_SHAPE. */
enum fiunet_packing10 { FIUNET_PACK10_V210 = 0, FIUNET_PACK10_Y210 = 1, FIUNET_PACK10_P210 = 2 };
int fiunet_unpack_422p10(const void* in, int packing, const fiunet_packed_layout* in_packed,
                         const fiunet_surface_layout* in_surface, uint16_t* out, size_t out_frame_stride, int B, int H,
                         int W, void* stream);
int fiunet_pack_422p10(const uint16_t* in, size_t in_frame_stride, void* out, int packing,
                       const fiunet_packed_layout* out_packed, const fiunet_surface_layout* out_surface, int B, int H,
                       int W, void* stream);

/* Scene cuts in the video loops (ABI v8, added without a version bump: nothing existing changed).  The reference has
 * no video loop; the definition is our own.  For N frames and the N-1 intervals i between F[i] and
 * F[i+1]: sad[i] = sum over every sample of |F[i+1] - F[i]| (exact int64; 10-bit samples above 1023 read as 1023),
 * mafd[i] = sad[i] * 100.0 / count / 2^bits in IEEE double in that order (count = samples per frame, all planes),
 * score[i] = min(mafd[i], |mafd[i] - mafd[i-1]|, |mafd[i] - mafd[i+1]|) (a missing neighbour left out), and interval
 * i is a cut iff score[i] >= threshold.  Device pointers; asynchronous on `stream`; no allocation, no
 * synchronisation; n_frames < 2 is a no-op.  FIUNET_ERR_INVALID_ARG on NULL pointers or n_frames < 0. */
/* ACCUMULATES sad[i] into sums[n_frames - 1] (zeroed by the caller): `frames` is a contiguous stack of n_frames frames
 * of frame_samples samples, so one sad can span several planar stacks (Y, U, V) of the same frames. */
int fiunet_pair_sad_u8(const uint8_t* frames, int n_frames, size_t frame_samples, int64_t* sums, void* stream);
int fiunet_pair_sad_p10(const uint16_t* frames, int n_frames, size_t frame_samples, int64_t* sums, void* stream);
/* sums[n_frames - 1] -> scores[n_frames - 1] (double) and flags[n_frames - 1] (1 = cut).  count = samples per frame
 * over every stack that went into the sums; bits 8 or 10; threshold in (0, 100] (NaN rejected). */
int fiunet_scene_cuts(const int64_t* sums, int n_frames, size_t count, int bits, double threshold, double* scores,
                      uint8_t* flags, void* stream);
/* Sample-and-hold on the interleaved result of a factor-`factor` loop over n_frames input frames ((n_frames - 1) *
 * factor + 1 frames of frame_bytes bytes, contiguous): for every i with flags[i] != 0, frames i*factor + 1 ..
 * i*factor + factor - 1 become byte copies of frame i*factor.  Bytes, so every sample depth shares it.  The flags are
 * read on the device.  factor: a power of two in [2, 2^20]. */
int fiunet_hold_cut_frames(uint8_t* video, int n_frames, size_t frame_bytes, int factor, const uint8_t* flags,
                           void* stream);

/* Frame-rate conversion (ABI v8, added without a version bump: nothing existing changed).  `grid` holds
 * the frames of a `depth`-level bisection, G = 2^depth: [(n_intervals << depth) + 1][frame_samples], row k*G + m at
 * clip time first_interval + k + m / G.  With source rate / target rate = p / q reduced (0 < p < q <= 2^20), output
 * row k is clip output frame j = j0 + k at time j * p / q: i = j*p / q, r = j*p % q, lo = r*G / q, wn = r*G % q, and
 *   mode 0 (blend)    out = (A * (q - wn) + B * wn + q / 2) / q per sample in integers, A = the grid row at time
 *                     i + lo / G, B the row after it; 10-bit words above 1023 read as 1023; wn == 0: a byte copy of A
 *   mode 1 (nearest)  a byte copy of B if 2 * wn > q, else of A
 *   cut               flags != NULL, flags[i - first_interval] != 0 and r != 0: a byte copy of the grid row at time i
 * flags: [n_intervals] on the device (read there), or NULL.  out: [n_out][frame_samples].  Device pointers;
 * asynchronous on `stream`; no allocation, no synchronisation; n_out == 0 is a no-op.  FIUNET_ERR_INVALID_ARG, checked
 * on the host before any launch: NULL grid / out, depth outside 1..4, p == 0, p >= q, q > 2^20, a mode other than 0 /
 * 1, a negative count, or a first / last requested frame whose rows fall outside the grid. */
int fiunet_retime_u8(const uint8_t* grid, int n_intervals, size_t frame_samples, int depth, uint64_t first_interval,
                     uint64_t j0, int n_out, uint32_t p, uint32_t q, int mode, const uint8_t* flags, uint8_t* out,
                     void* stream);
int fiunet_retime_p10(const uint16_t* grid, int n_intervals, size_t frame_samples, int depth, uint64_t first_interval,
                      uint64_t j0, int n_out, uint32_t p, uint32_t q, int mode, const uint8_t* flags, uint16_t* out,
                      void* stream);

/* Repeated frames in video (ABI v8, added without a version bump: nothing existing changed).
 * peak[i] = the largest sum of |F[i+1] - F[i]| over the aligned 64-sample segments of a frame of frame_samples samples,
 * counted from its first sample (the last segment may be short; 10-bit samples above 1023 read as 1023): a frame-wide
 * mean hides a small moving object, a maximum over short segments does not.  MAX-ACCUMULATES into peaks[n_frames - 1]
 * (uint32, zeroed by the caller), so several planar stacks of the same frames can share one result.  Exact in any order.
 * Calling conventions of fiunet_pair_sad_*: device pointers, asynchronous on `stream`, no allocation, no
 * synchronisation, n_frames < 2 is a no-op, FIUNET_ERR_INVALID_ARG on NULL pointers or n_frames < 0. */
int fiunet_pair_peak_u8(const uint8_t* frames, int n_frames, size_t frame_samples, uint32_t* peaks, void* stream);
int fiunet_pair_peak_p10(const uint16_t* frames, int n_frames, size_t frame_samples, uint32_t* peaks, void* stream);

/* Table-driven resampling: output row k of out[n_out][frame_samples] is, with e = entries[k] and A = row e.row of
 * grid[n_rows][frame_samples], B the row after it,
 *   e.wn == 0   a byte copy of A (B is not read)
 *   else        (A * (e.den - e.wn) + B * e.wn + e.den / 2) / e.den per sample in integers; 10-bit words above 1023
 *               read as 1023
 * `entries` is HOST memory, read during the call: every entry is checked before the first launch and the entries
 * travel in the kernels' arguments (64 output frames per launch), so there is no device table and no copy, nothing of
 * the array is needed once the call has returned, and the call can be captured into a graph.  grid and out are device
 * pointers; asynchronous on `stream`; no allocation, no synchronisation; n_out == 0 is a no-op.
 * FIUNET_ERR_INVALID_ARG, before any launch and before a pointer is used: NULL grid / out / entries, a negative count,
 * or an entry with row >= n_rows, wn >= den, wn > 0 and row + 1 >= n_rows, or den outside 1 .. 2^20. */
typedef struct fiunet_retime_entry {
    uint32_t row, wn, den;
} fiunet_retime_entry;
int fiunet_retime_table_u8(const uint8_t* grid, int n_rows, size_t frame_samples, const fiunet_retime_entry* entries,
                           int n_out, uint8_t* out, void* stream);
int fiunet_retime_table_p10(const uint16_t* grid, int n_rows, size_t frame_samples, const fiunet_retime_entry* entries,
                            int n_out, uint16_t* out, void* stream);

/* A synthesized shutter (ABI v8, added without a version bump: nothing existing changed; csrc/shutter.hip.h, DESIGN.md
 * 3.3y): conversion to a lower frame rate averages the clip over the time the slower camera's shutter is open.  Output
 * row k of out[n_out][frame_samples] is a weighted mean of consecutive rows of grid[n_rows][frame_samples].  `entries` is
 * a run of 32-bit words, per output frame
 *   first_row, n_taps, w[0] .. w[n_taps - 1]        (n_taps + 2 words; the next frame's entry follows at once)
 * and the frame is, per sample in integers,
 *   (sum_t w[t] * grid[first_row + t] + 2^19) >> 20   with sum_t w[t] == 2^20; 10-bit words above 1023 read as 1023
 *   a byte copy of the row whose weight is 2^20        (one live tap; words above 1023 stay as they are)
 * A row whose weight is 0 is not read.  `entries` is HOST memory, read during the call: every entry is checked before the
 * first launch (n_taps before the weights behind it are read) and the entries travel in the kernels' arguments (up to 32
 * output frames and 864 weights per launch), so there is no device table and no copy, nothing of the array is needed once
 * the call has returned, and the call can be captured into a graph.  grid and out are device pointers; asynchronous on
 * `stream`; no allocation, no synchronisation; n_out == 0 is a no-op.
 * FIUNET_ERR_INVALID_ARG, before any launch and before a pointer is used: NULL grid / out / entries, a negative count, or
 * an entry with n_taps outside 1 .. 48, first_row + n_taps > n_rows, or weights that do not sum to 2^20. */
int fiunet_shutter_u8(const uint8_t* grid, int n_rows, size_t frame_samples, const uint32_t* entries, int n_out,
                      uint8_t* out, void* stream);
int fiunet_shutter_p10(const uint16_t* grid, int n_rows, size_t frame_samples, const uint32_t* entries, int n_out,
                       uint16_t* out, void* stream);

/* Resize of frame planes, bilinear or by area (csrc/resize.hip.h).  A plane is described in SAMPLES of its buffer:
 * sample (y, x) of frame f lies at offset + f * frame_stride + y * pitch + x * step.  Plane i of `src_planes` is
 * resampled into plane i of `dst_planes`, each pair on its own grid, for n_frames frames, in one launch per 2^31 store
 * chunks (the descriptors travel in the kernel's arguments: `src_planes` / `dst_planes` are HOST memory, read during the
 * call; there is no device table, no workspace and no copy, and the call can be captured into a graph).
 *   8 bits    imageio_lite.resize_linear_u8 to the last bit: half-pixel centres, the coordinate in fp64 rounded to
 *             fp32, 11-bit coefficients, OpenCV's two-stage vertical rounding (the project's statement of
 *             cv2.resize(INTER_LINEAR) on uchar; not pinned against OpenCV itself)
 *   10 bits   the same taps; samples above 1023 read as 1023; out = min((b0 * S0 + b1 * S1 + 2^21) >> 22, 1023)
 *   equal h and w: a copy of the plane, sample for sample
 * Asynchronous on `stream`; no allocation, no synchronisation; n_frames == 0 is a no-op.  FIUNET_ERR_INVALID_ARG, before
 * any launch and before a device pointer is used: NULL pointers (a uint16_t pointer that is not 2-byte aligned), n_planes
 * outside 1..4, n_frames < 0, a size outside 1 .. 2^24, a step outside 1..4, pitch < (w - 1) * step + 1, a plane that
 * does not lie inside its frame stride (offset + (h - 1) * pitch + (w - 1) * step + 1 > frame_stride), or source and
 * destination byte ranges (first sample of any plane of frame 0 to the last of frame n_frames - 1) that overlap.
 * FIUNET_ERR_UNSUPPORTED: a destination plane of 2^31 or more 16-byte store chunks.
 *
 * The filter is the `filter` member of the DESTINATION planes, which must agree within a call; source planes carry 0.  A
 * source filter other than 0, a destination filter that is neither value below, or destination planes that disagree are
 * FIUNET_ERR_INVALID_ARG, before any launch.  FIUNET_RESIZE_LINEAR (0) is everything above.  FIUNET_RESIZE_AREA is the
 * alias-free down-scaling filter, in integers, at 8 and 10 bits alike (tests/resize_area_ref.py):
 *   axis      n_src -> n_dst, n_dst <= n_src, in units of 1 / n_dst of a source sample: destination index d covers
 *             [d * n_src, (d + 1) * n_src), source index j covers [j * n_dst, (j + 1) * n_dst), and the weight is the
 *             length of the overlap, w(d, j) = max(0, min((d + 1) * n_src, (j + 1) * n_dst) - max(d * n_src, j * n_dst));
 *             the weights of one d sum to n_src
 *   plane     source sh x sw, destination dh x dw: N = sum_y wy(r, y) * sum_x wx(c, x) * v(y, x), D = sw * sh,
 *             out = (N + D / 2) / D in integer division: exact, half up; samples above 1023 read as 1023 at 10 bits
 *   equal h and w: the same copy as under the linear filter
 * A constant plane stays constant; for whole ratios rx, ry it is the rounded mean of each rx x ry block.  Two refusals of
 * its own, before any launch: a plane pair with a destination wider or taller than its source is FIUNET_ERR_INVALID_ARG
 * (the area filter only down-scales: enlarge with the linear filter), and a ratio above 64 on either axis (sw > 64 * dw
 * or sh > 64 * dh) is FIUNET_ERR_UNSUPPORTED (one thread sums at most 66 x 66 samples). */
enum fiunet_resize_filter {
    FIUNET_RESIZE_LINEAR = 0,
    FIUNET_RESIZE_AREA = 1
};
typedef struct fiunet_resize_plane {
    size_t offset, pitch, frame_stride;
    int32_t h, w, step, filter;   /* filter: a fiunet_resize_filter in a destination plane, 0 in a source plane */
} fiunet_resize_plane;
int fiunet_resize_planes_u8(const uint8_t* src, const fiunet_resize_plane* src_planes, uint8_t* dst,
                            const fiunet_resize_plane* dst_planes, int n_planes, int n_frames, void* stream);
int fiunet_resize_planes_p10(const uint16_t* src, const fiunet_resize_plane* src_planes, uint16_t* dst,
                             const fiunet_resize_plane* dst_planes, int n_planes, int n_frames, void* stream);

/* Replaces preprocess_image's arithmetic (model/inference.py:31-35): out = 2*(in/255) - 1. */
int fiunet_preprocess_u8(const uint8_t* in, float* out, size_t n, void* stream);
/* Replaces postprocess_image's arithmetic (model/inference.py:54-61), truncating cast. */
int fiunet_postprocess_u8(const float* in, uint8_t* out, size_t n, void* stream);

/* Quality metrics of the evaluation loop on device.  The reference computes
 * them on the host with scikit-image, one frame at a time (model/evaluation.py:194-218,
 * model/evaluation_simple.py:134-156): peak_signal_noise_ratio(target, pred, data_range=255) and
 * structural_similarity(target, pred, data_range=255) with skimage's defaults (7x7 uniform window,
 * sample covariance, K1 = 0.01, K2 = 0.03, mean over the image minus a 3-pixel border).
 * pred, target: device uint8, `images` planes of H x W (e.g. the [B, C, H, W] output of
 * fiunet_forward_u8 and the ground-truth frames); out: device double[images] (+inf PSNR for identical
 * planes, as skimage).  workspace: device scratch of fiunet_metrics_workspace_bytes(images, H, W),
 * 256-B aligned.  SSIM needs H, W >= 7.  Asynchronous on `stream`. */
size_t fiunet_metrics_workspace_bytes(int images, int H, int W);
int fiunet_psnr_u8(const uint8_t* pred, const uint8_t* target, int images, int H, int W, double* out,
                   void* workspace, size_t workspace_bytes, void* stream);
int fiunet_ssim_u8(const uint8_t* pred, const uint8_t* target, int images, int H, int W, double* out,
                   void* workspace, size_t workspace_bytes, void* stream);

/* The same two metrics on planes where they lie (hold-out scoring of video: the Y, U and V planes of packed 4:2:0
 * rows, every second row of a stack): `images` planes of H x W samples, image i of `pred` at pred + i *
 * pred_image_stride, its rows pred_row_pitch apart; strides and pitches in SAMPLES.  bits 8: uint8_t samples, peak 255
 * (on contiguous planes the values are fiunet_psnr_u8's / fiunet_ssim_u8's to the last bit); bits 10: uint16_t words of
 * 10-bit codes, peak 1023 (a word above 1023 reads as 1023, as in the 10-bit conversions).  pred and target may point
 * into one allocation.  out_psnr / out_ssim: device double[images]; out_sse (may be NULL): device uint64[images], the
 * exact sum of squared differences PSNR = 10 log10(peak^2 / (sse / (H*W))) is made from (+inf at 0).  SSIM: the
 * definition above with C1 = (0.01 peak)^2, C2 = (0.03 peak)^2; exact integer window sums, fp64 map and mean in a
 * fixed order.  workspace: fiunet_plane_metrics_workspace_bytes(images, H, W), 256-B aligned.  Asynchronous on
 * `stream`; no allocation, no synchronisation.  FIUNET_ERR_INVALID_ARG, before any launch and before any pointer is
 * used: NULL pointers, bits not 8 or 10, images / H / W < 1 (SSIM: H or W < 7), more than 65535 images, a row pitch
 * < W, images > 1 with an image stride smaller than one plane ((H-1) * pitch + W), a workspace that is too small or
 * not aligned. */
size_t fiunet_plane_metrics_workspace_bytes(int images, int H, int W);
int fiunet_plane_psnr(const void* pred, size_t pred_image_stride, size_t pred_row_pitch,
                      const void* target, size_t target_image_stride, size_t target_row_pitch,
                      int bits, int images, int H, int W, double* out_psnr, unsigned long long* out_sse,
                      void* workspace, size_t workspace_bytes, void* stream);
int fiunet_plane_ssim(const void* pred, size_t pred_image_stride, size_t pred_row_pitch,
                      const void* target, size_t target_image_stride, size_t target_row_pitch,
                      int bits, int images, int H, int W, double* out_ssim,
                      void* workspace, size_t workspace_bytes, void* stream);

/* The plane metrics on INTERLEAVED samples (hold-out scoring of raw video: U V of NV12, the bytes of packed RGB, the
 * byte positions of uyvy422 / yuyv422), with the depths, peaks and conventions of the two entry points above.
 *
 * fiunet_interleaved_psnr: an image is H rows of W * components samples, components S in {2, 3, 4}; the sample at
 * position p of a row belongs to component p % S.  One pass over the bytes gives all S components: out_psnr is device
 * double[images * S], out_sse (may be NULL) device uint64[images * S], both image-major (image i, component c at
 * i * S + c); the mean is over the H*W samples of a component.  A component's PSNR and sse are, to the last bit, what
 * fiunet_plane_psnr gives on a contiguous copy of that component.  Strides and pitches in samples; a row pitch below
 * W * S is refused, as is images > 1 with an image stride below (H-1) * pitch + W*S, components outside 2..4 and
 * images * S > 65535.  workspace: fiunet_plane_metrics_workspace_bytes(images * S, H, W) (there is no size function
 * of its own), 256-B aligned.
 *
 * fiunet_stepped_ssim: fiunet_plane_ssim with a sample step in {1, 2, 3, 4} on each side: sample (y, x) of an
 * image lies at y * row_pitch + x * step.  fiunet_plane_ssim is step 1 of the same kernel.  A row pitch below
 * (W-1) * step + 1 is refused, as is images > 1 with an image stride below (H-1) * pitch + (W-1) * step + 1.
 * workspace: fiunet_plane_metrics_workspace_bytes(images, H, W).
 *
 * Both: asynchronous on `stream`, no allocation, no synchronisation; every refusal is FIUNET_ERR_INVALID_ARG before any
 * launch and before any pointer is used. */
int fiunet_interleaved_psnr(const void* pred, size_t pred_image_stride, size_t pred_row_pitch,
                            const void* target, size_t target_image_stride, size_t target_row_pitch,
                            int bits, int components, int images, int H, int W, double* out_psnr,
                            unsigned long long* out_sse, void* workspace, size_t workspace_bytes, void* stream);
int fiunet_stepped_ssim(const void* pred, size_t pred_image_stride, size_t pred_row_pitch, int pred_step,
                              const void* target, size_t target_image_stride, size_t target_row_pitch, int target_step,
                              int bits, int images, int H, int W, double* out_ssim,
                              void* workspace, size_t workspace_bytes, void* stream);

/* The classical motion-compensated baseline of the evaluators on device: dense Farneback flow with the
 * reference's parameters (model/evaluation_simple.py:76-103: pyr_scale 0.5, 3 levels, winsize 15, 3 iterations, poly_n 5,
 * poly_sigma 1.1, flags 0; the definition is the package's optical_flow.py, parity-unpinned against OpenCV) and remap's
 * fixed-point bilinear warp along it.
 * fiunet_farneback_flow: prev, next: B frames of H x W samples each, frame i at base + i * image_stride, rows row_pitch
 * apart, both in SAMPLES and the same for both (bits 8: uint8_t; bits 10: uint16_t words of 10-bit codes, which enter
 * the flow as code / 4).  flow_out: device float [B, H, W, 2] = (dx, dy) of prev -> next, 8-byte aligned.  workspace:
 * fiunet_flow_workspace_bytes(B, H, W) (0 for bad arguments), 256-B aligned.  A pair's flow does not depend on B or on
 * its place in the batch.
 * fiunet_flow_warp: one plane of B frame pairs along `flow` [B, flow_h, flow_w, 2]; where flow_h x flow_w is not H x W
 * (the luma flow, a sub-sampled chroma plane) the flow is resampled to the plane first (cv2.resize's linear rule) and
 * scaled by W / flow_w and H / flow_h.  FIUNET_FLOW_REFERENCE: frame0 at p + flow(p) / 2, the reference's formula (it
 * samples AGAINST the motion); frame1 is not read but must not be NULL.  FIUNET_FLOW_MOTION: (frame0 at p - flow(p) / 2
 * + frame1 at p + flow(p) / 2 + 1) >> 1.  Coordinates are clamped to the plane in fp32, rounded half-to-even to 1/32
 * pixel and sampled with 15-bit integer weights, (acc + 2^14) >> 15.  out: samples of the same depth with its own
 * strides; it must not overlap the frames.
 * Both: asynchronous on `stream`; no allocation, no synchronisation.  Before any launch: NULL pointers, bits not 8 or
 * 10, a bad mode, B / H / W < 1, B > 4096, a side above 32768, a row pitch < W, B > 1 with an image stride smaller than
 * one frame and misaligned pointers are FIUNET_ERR_INVALID_ARG; a workspace that is too small is FIUNET_ERR_WORKSPACE. */
enum fiunet_flow_mode { FIUNET_FLOW_REFERENCE = 0, FIUNET_FLOW_MOTION = 1 };
size_t fiunet_flow_workspace_bytes(int B, int H, int W);
int fiunet_farneback_flow(const void* prev, const void* next, int bits, int B, int H, int W, size_t image_stride,
                          size_t row_pitch, float* flow_out, void* workspace, size_t workspace_bytes, void* stream);
int fiunet_flow_warp(const void* frame0, const void* frame1, const float* flow, int mode, int bits, int B, int H, int W,
                     size_t image_stride, size_t row_pitch, int flow_h, int flow_w, void* out, size_t out_image_stride,
                     size_t out_row_pitch, void* stream);

/* Motion-compensated resampling (retime "motion"; added without a version bump): ONE PLANE of n_out
 * output frames, each warped along the flow between two neighbouring rows of a grid of n_rows frames to its own time.
 * A plane is a fiunet_resize_plane (samples of its buffer; filter 0): `grid_plane` lies in `grid`, `out_plane`, of the
 * same h x w, in `out`, so the U / V of NV12, the bytes of packed RGB and the capture formats are read and written where
 * they lie.  Output frame k is e = entries[k]: A = grid row e.row, B = the row after it, (dx, dy) = field e.flow of
 * `flow` [n_flows, flow_h, flow_w, 2] (A -> B on the lead plane) at the sample, resampled and scaled as in
 * fiunet_flow_warp where flow_h x flow_w is not h x w; s0 = fp32(wn / den), s1 = fp32((den - wn) / den), each computed
 * in double and rounded once:
 *   a   = remap(A, clamp(x - s0 * dx, 0, w - 1), clamp(y - s0 * dy, 0, h - 1))
 *   b   = remap(B, clamp(x + s1 * dx, 0, w - 1), clamp(y + s1 * dy, 0, h - 1))
 *   out = ((den - wn) * a + wn * b + den / 2) / den      in integer division
 * every product rounded to fp32, then every sum (no fused multiply-add); remap as in fiunet_flow_warp (1/32 pixel, 15-bit
 * weights, (acc + 2^14) >> 15; 10-bit words above 1023 read as 1023; a NaN flow clamps to coordinate 0).  2 * wn == den
 * is FIUNET_FLOW_MOTION to the last bit, an all-zero flow is the blend of fiunet_retime_table_*; wn == 0 copies the
 * samples of A as they are stored.  e.flag: FIUNET_WARP_NO_FLAG, or an index into the device array `flags` [n_flags]
 * (NULL with n_flags 0): a frame whose flag is non-zero on the device is NOT WRITTEN.  Samples of `out` outside the
 * plane are never written.  `entries` and the planes are HOST memory, read during the call; the entries travel in the
 * kernel's arguments, 64 output frames per launch: no device table, no allocation, no synchronisation, capturable.
 * A pair's flow does not depend on its batch (fiunet_farneback_flow), so neither does a frame made here.
 * FIUNET_ERR_INVALID_ARG, before any launch and before a pointer is used: NULL grid / out / planes / flow (entries with
 * n_out > 0; flags with n_flags > 0), a uint16_t pointer that is not 2-byte aligned, a negative count, a plane that
 * breaks fiunet_resize_planes' rules (sizes, step 1..4, pitch, inside its frame stride) or has a side above 32768 or a
 * filter other than 0, planes of different h x w, a bad flow shape, flow not 8-byte aligned, an entry with
 * row + 1 >= n_rows, flow >= n_flows, wn >= den, den outside 1 .. 2^20 or a flag outside -1 .. n_flags - 1, and an
 * out plane range that overlaps the grid plane's. */
#define FIUNET_WARP_NO_FLAG (-1)
typedef struct fiunet_warp_entry {
    uint32_t row, wn, den, flow;
    int32_t flag;
} fiunet_warp_entry;
int fiunet_warp_table_u8(const uint8_t* grid, int n_rows, const fiunet_resize_plane* grid_plane, const float* flow,
                              int n_flows, int flow_h, int flow_w, const uint8_t* flags, int n_flags,
                              const fiunet_warp_entry* entries, int n_out, uint8_t* out,
                              const fiunet_resize_plane* out_plane, void* stream);
int fiunet_warp_table_p10(const uint16_t* grid, int n_rows, const fiunet_resize_plane* grid_plane, const float* flow,
                               int n_flows, int flow_h, int flow_w, const uint8_t* flags, int n_flags,
                               const fiunet_warp_entry* entries, int n_out, uint16_t* out,
                               const fiunet_resize_plane* out_plane, void* stream);

/* Motion-guided chroma for the grayscale video route (added without a version bump; the definition is
 * the package's chroma.py).  One inserted frame M between the stored frames A and B: M's luma comes from the network, and
 * its chroma is, 8x8 luma block by block, the warp of A's and B's chroma to the middle of the interval along the luma flow
 * A -> B, or their rounded average, whichever the network's luma says fits there.
 * fiunet_chroma_pick_*: n frames.  a, b, m: the luma of A, B and M, each a fiunet_resize_plane (filter 0) in a buffer of
 * its own or at another offset of the same one, all of one h x w; frame k of a plane lies k * frame_stride on.  `field`:
 * device float [n, h, w, 2], the flow A -> B on the luma (fiunet_farneback_flow), 8-byte aligned.  With
 * Ym = fiunet_warp_table_* at wn = 1, den = 2 and Ya = (A + B + 1) >> 1, block (by, bx) of the ceil(h / 8) x ceil(w / 8)
 * blocks has cost_m = sum |Ym - M| and cost_a = sum |Ya - M| over rows 8 by - 4 .. 8 by + 11 and columns
 * 8 bx - 4 .. 8 bx + 11, every index clamped to the plane (a clamped index counts again: 256 terms); pick [n, ceil(h / 8),
 * ceil(w / 8)] uint8 = 1 iff cost_m < cost_a (a tie takes the average).  10-bit words above 1023 read as 1023.
 * fiunet_chroma_fill_*: both chroma planes of n frames.  a_planes, b_planes, out_planes: two planes each (U, V), all six
 * of one h x w, sub-sampled against the luma by (sy, sx), each 1 or 2; `field` [n, field_h, field_w, 2] and `pick`
 * [n, ceil(field_h / 8), ceil(field_w / 8)] as above, field_h x field_w the luma size.  Sample (cy, cx) is, where
 * pick[(cy * sy) >> 3][(cx * sx) >> 3] is non-zero, what fiunet_warp_table_* writes for wn = 1, den = 2 (the field
 * resampled to the chroma plane by that call's rule), to the last bit; elsewhere (A + B + 1) >> 1.  Samples of `out`
 * outside its planes are never written.
 * Both: the planes are HOST memory, read during the call; asynchronous on `stream`, no allocation, no synchronisation,
 * capturable; n == 0 is a no-op.  FIUNET_ERR_INVALID_ARG, before any launch and before a pointer is used: a NULL
 * argument, a uint16_t pointer that is not 2-byte aligned, n outside 0 .. 4096, a plane that breaks
 * fiunet_warp_table_*'s plane rules, planes of different h x w, `field` not 8-byte aligned, a plane range that leaves the
 * address space, pick overlapping a luma plane; for the fill also sy or sx other than 1 or 2, a bad field shape, a
 * chroma plane with (h - 1) * sy >= field_h or (w - 1) * sx >= field_w, out's planes overlapping each other or A's or
 * B's. */
int fiunet_chroma_pick_u8(const uint8_t* a, const fiunet_resize_plane* a_plane, const uint8_t* b,
                          const fiunet_resize_plane* b_plane, const uint8_t* m, const fiunet_resize_plane* m_plane,
                          const float* field, int n, uint8_t* pick, void* stream);
int fiunet_chroma_pick_p10(const uint16_t* a, const fiunet_resize_plane* a_plane, const uint16_t* b,
                           const fiunet_resize_plane* b_plane, const uint16_t* m, const fiunet_resize_plane* m_plane,
                           const float* field, int n, uint8_t* pick, void* stream);
int fiunet_chroma_fill_u8(const uint8_t* a, const fiunet_resize_plane* a_planes, const uint8_t* b,
                          const fiunet_resize_plane* b_planes, const float* field, int field_h, int field_w,
                          const uint8_t* pick, int sy, int sx, int n, uint8_t* out, const fiunet_resize_plane* out_planes,
                          void* stream);
int fiunet_chroma_fill_p10(const uint16_t* a, const fiunet_resize_plane* a_planes, const uint16_t* b,
                           const fiunet_resize_plane* b_planes, const float* field, int field_h, int field_w,
                           const uint8_t* pick, int sy, int sx, int n, uint16_t* out,
                           const fiunet_resize_plane* out_planes, void* stream);

/* Deinterlacing (added without a version bump: nothing existing changed).  An interlaced frame holds two
 * fields taken half a frame period apart: FIUNET_DEINT_TFF, the even rows come first in time; FIUNET_DEINT_BFF, the odd
 * rows.  Field i (0: the first in time) of a frame keeps the rows of parity p = (order == BFF) ^ i, which are copied; the
 * rows of the other parity are filled in.  The definition is the project's own, in integers, in the spirit of yadif and
 * not pinned against ffmpeg; tests/deinterlace_ref.py states it in numpy and the kernels equal it bit for bit.  With
 * cur = F[t], prev = F[t - 1], next = F[t + 1], (prev2, next2) = (prev, cur) for i == 0 and (cur, next) for i == 1,
 * ym = y - 1 (y + 1 at y == 0), yp = y + 1 (y - 1 at y == h - 1), all in int32:
 *   c = cur[ym][x], e = cur[yp][x], pred = (c + e) >> 1                                   FIUNET_DEINT_BOB writes pred
 *   d = (prev2[y][x] + next2[y][x]) >> 1, t0 = |prev2[y][x] - next2[y][x]|,
 *   t1 = (|prev[ym][x] - c| + |prev[yp][x] - e|) >> 1, t2 the same with next, diff = max(t0 >> 1, t1, t2)
 *   where 3 <= x < w - 3: S(j) = sum over k = -1, 0, 1 of |cur[ym][x + k + j] - cur[yp][x + k - j]|, score = S(0) - 1;
 *     if S(-1) < score: score = S(-1), pred = (cur[ym][x - 1] + cur[yp][x + 1]) >> 1, and only then j = -2 the same way;
 *     then j = +1 and, if it was taken, j = +2, against the score as it stands
 *   unless FIUNET_DEINT_NO_SPATIAL_CHECK, where 2 <= y < h - 2: b = (prev2[y - 2][x] + next2[y - 2][x]) >> 1, f the same
 *     at y + 2, mx = max(d - e, d - c, min(b - c, f - e)), mn = min(d - e, d - c, max(b - c, f - e)),
 *     diff = max(diff, mn, -mx)
 *   out = min(max(pred, d - diff), d + diff)
 * A result lies between the smallest and the largest input sample: 16-bit words are neither masked nor clamped.
 * `src` is a window of n_src frames; frames first .. first + n_frames - 1 of it are deinterlaced, and their neighbours
 * t - 1 and t + 1 come from the window, clamped to 0 .. n_src - 1: a streaming caller hands over one context frame either
 * side, and at the ends of a clip the clamp is the definition itself.  FIUNET_DEINT_FIELD_RATE: dst receives 2 * n_frames
 * frames, frame 2 * k + i from field i of window frame first + k; FIUNET_DEINT_FRAME_RATE: n_frames frames, each from
 * field 0.  method_flags: FIUNET_DEINT_ADAPTIVE or FIUNET_DEINT_BOB, or-ed with FIUNET_DEINT_NO_SPATIAL_CHECK or not.
 * Planes: 1..4 fiunet_resize_plane pairs (HOST memory, read during the call; filter 0; step 1..4), plane i of src_planes
 * in `src` and of dst_planes in `dst`, of one h x w; every plane is filtered on its own with the same p, so the U and V of
 * NV12, the bytes of uyvy422 and packed RGB are filtered where they lie.  Samples of dst outside its planes are never
 * written.  Step-1 planes whose bases, pitches and frame strides are multiples of 16 bytes on both sides take a path of
 * 16-byte accesses; every other plane is computed sample by sample, to the same bits.
 * Asynchronous on `stream`, no allocation, no synchronisation, capturable; n_frames == 0 is a no-op.
 * FIUNET_ERR_INVALID_ARG, before any launch and before a pointer is used: a NULL argument, a uint16_t pointer that is not
 * 2-byte aligned, n_planes outside 1..4, an unknown order, rate or method_flags, first or n_frames outside the window,
 * more than 65535 output frames, a plane that breaks fiunet_resize_planes' rules or has filter != 0 or h < 2, a plane pair
 * of different h x w, a plane range that leaves the address space, dst's planes overlapping src's. */
enum fiunet_deint {
    FIUNET_DEINT_TFF = 0, FIUNET_DEINT_BFF = 1,                  /* order */
    FIUNET_DEINT_FIELD_RATE = 0, FIUNET_DEINT_FRAME_RATE = 1,    /* rate */
    FIUNET_DEINT_ADAPTIVE = 0, FIUNET_DEINT_BOB = 1,             /* method_flags: the method ... */
    FIUNET_DEINT_NO_SPATIAL_CHECK = 256                          /* ... and this flag */
};
int fiunet_deinterlace_u8(const uint8_t* src, int n_src, const fiunet_resize_plane* src_planes, uint8_t* dst,
                          const fiunet_resize_plane* dst_planes, int n_planes, int first, int n_frames, int order, int rate,
                          int method_flags, void* stream);
int fiunet_deinterlace_p10(const uint16_t* src, int n_src, const fiunet_resize_plane* src_planes, uint16_t* dst,
                           const fiunet_resize_plane* dst_planes, int n_planes, int first, int n_frames, int order, int rate,
                           int method_flags, void* stream);

/* Inverse telecine (added without a version bump: nothing existing changed).  Hard-telecined film - 24 fps
 * carried as 29.97 fps interlaced video by 2:3 pulldown - holds every film frame whole, but two of every five video frames
 * are woven from the fields of two different film frames.  The two kernels here score the three field pairings of a frame
 * and weave the chosen fields; the choice and the decimation are host arithmetic on the scores (stated below for the
 * record, done by the caller).  The definition is the project's own, in integers, in the spirit of ffmpeg's fieldmatch +
 * decimate and not pinned against ffmpeg; tests/ivtc_ref.py states it in numpy and the kernels equal it bit for bit.
 *   candidates  frame F[t] of field order `order` keeps the rows of its first field's parity k (FIUNET_DEINT_TFF: 0, the
 *               even rows; FIUNET_DEINT_BFF: 1); the other rows come from F[t - 1] (candidate p), F[t] (c) or F[t + 1]
 *               (n), t - 1 and t + 1 clamped to the window 0 .. n_src - 1; every plane of a frame uses the same choice
 *   comb score  of a candidate W on an h x w plane, h >= 3, in int32: for 1 <= y <= h - 2 and every x, with u = W[y-1][x],
 *               m = W[y][x], d = W[y+1][x] (10-bit words above 1023 read as 1023), the sample is combed iff
 *               (u - m) * (d - m) > T * T, T = threshold in 0..1023 (the Python default: 12 at 8 bits, 48 at 10).  The
 *               plane is cut into blocks of 16 rows x 64 columns aligned to its origin (row y in block row y / 16; the
 *               last block row and column may be partial); the score is the LARGEST count of combed samples of a block,
 *               so that a small moving object shows, as in fiunet_pair_peak_u8.  uint32, exact in any order
 *   choice      scores (sp, sc, sn): c if sc <= min(sp, sn), else p if sp <= sn, else n (ties prefer c, then p); a frame
 *               whose chosen score exceeds `combed` (default 48) is an orphan field at an edit or true interlaced video,
 *               and is replaced by fiunet_deinterlace_u8 / _p10 of F[t] (frame rate, adaptive) or kept as woven
 *   decimation  cycles of `cycle` (5) frames aligned to the clip's frame index; in every complete cycle the output frame
 *               with the smallest fiunet_pair_peak_u8 / _p10 value against the output frame before it (the whole tight
 *               frame; the clip's first frame counts as infinite; ties drop the earliest) is dropped, a trailing incomplete
 *               cycle is kept whole, and the rate becomes rate * (cycle - 1) / cycle
 * fiunet_field_match_u8 / _p10: `src` is a window of n_src frames; the three scores of frames first .. first + n_frames - 1
 * on `plane` (ONE fiunet_resize_plane in HOST memory, read during the call; filter 0; step 1..4: the luma of uyvy422, the Y
 * of NV12 or a byte of packed RGB serves where it lies) are MAX-ACCUMULATED into the device array `scores`
 * [n_frames][3], order p, c, n, which the caller zeroed: several planes may share one result, and the call captures into a
 * graph.  One launch computes the three candidates; step-1 planes whose base, pitch and frame stride are multiples of 16
 * bytes take a path of 16-byte loads, every other plane is read sample by sample, to the same bits.
 * fiunet_field_weave_u8 / _p10: output frame j of `dst`, j < n_out, takes the rows of parity `parity` (0: even, 1: odd) of
 * every plane from frame entries[j].keep of the window `src` and the other rows from frame entries[j].other; bytes are moved
 * and nothing else (16-bit words are not clamped), keep == other is a copy.  Planes: 1..4 fiunet_resize_plane pairs as
 * fiunet_deinterlace_u8 takes them.  `entries` is HOST memory, read during the call; every entry is checked before the
 * first launch, and the entries travel in the kernel's arguments, 64 output frames a launch.
 * Both: asynchronous on `stream`, no allocation, no synchronisation, capturable; no frames is a no-op.
 * FIUNET_ERR_INVALID_ARG, before any launch and before a pointer is used: a NULL argument, a misaligned pointer, an unknown
 * order or parity, a threshold outside 0..1023, first or n_frames outside the window, an entry that names a frame outside
 * the window, more than 65535 frames in one call, n_planes outside 1..4, a plane that breaks fiunet_resize_planes' rules
 * or has filter != 0, h < 3 (match) or h < 2 (weave), a plane pair of different h x w, a plane range that leaves the
 * address space, the destination (the scores; dst's planes) overlapping the source. */
typedef struct fiunet_weave_entry {
    uint32_t keep, other;
} fiunet_weave_entry;
int fiunet_field_match_u8(const uint8_t* src, int n_src, const fiunet_resize_plane* plane, int first, int n_frames,
                          int order, int threshold, uint32_t* scores, void* stream);
int fiunet_field_match_p10(const uint16_t* src, int n_src, const fiunet_resize_plane* plane, int first, int n_frames,
                           int order, int threshold, uint32_t* scores, void* stream);
int fiunet_field_weave_u8(const uint8_t* src, int n_src, const fiunet_resize_plane* src_planes, uint8_t* dst,
                          const fiunet_resize_plane* dst_planes, int n_planes, const fiunet_weave_entry* entries, int n_out,
                          int parity, void* stream);
int fiunet_field_weave_p10(const uint16_t* src, int n_src, const fiunet_resize_plane* src_planes, uint16_t* dst,
                           const fiunet_resize_plane* dst_planes, int n_planes, const fiunet_weave_entry* entries, int n_out,
                           int parity, void* stream);

/* The training loss' SSIM on device: SSIMLoss._ssim (model/train.py:37-56) - the
 * window_size x window_size Gaussian window (sigma 1.5, normalised as at train.py:27-35) applied as a
 * depth-wise conv2d with ZERO padding window_size//2 to img1, img2, img1^2, img2^2, img1*img2;
 * C1 = 0.01^2, C2 = 0.03^2; mean of the map.  img1, img2: device fp32, `images` planes of H x W (a
 * [B, C, H, W] tensor is B*C planes: the conv is depth-wise, so planes are independent), in the caller's
 * value range.  out_ssim: device double[images], the mean of each plane's SSIM map (all planes have H*W
 * pixels, so `ssim_map.mean()` (:54) is the mean of these and `.mean(1).mean(1).mean(1)` (:56) the mean
 * over a sample's C planes).  out_sqerr (may be NULL): device double[images], sum (img1 - img2)^2 of each
 * plane - CombinedLoss' MSE term (train.py:75-87) is their total / (images*H*W).  window_size must be odd
 * (the reference's default and only value is 11) and <= 31.  window_1d: HOST pointer to the window_size
 * normalised 1-D Gaussian weights the caller computed (train.py:27-29 with the caller's own torch, whose
 * reduction order decides the last bit of `gauss.sum()`), or NULL to have them computed here (sequential
 * fp32 sum; the mean SSIM then sits within ~1e-6 of the reference's).  Workspace:
 * fiunet_ssim_gauss_workspace_bytes(images, H, W), 256-B aligned.  Asynchronous on `stream`. */
size_t fiunet_ssim_gauss_workspace_bytes(int images, int H, int W);
int fiunet_ssim_gauss_f32(const float* img1, const float* img2, int images, int H, int W, int window_size,
                          const float* window_1d, double* out_ssim, double* out_sqerr, void* workspace,
                          size_t workspace_bytes, void* stream);

/* Parity-test hook: after a fiunet_forward on `workspace` (with FIUNET_OPT_KEEP_ALL set), convert one intermediate
 * activation (blocked channels-last in the compute precision; two-piece in BF16X2) to fp32 NCHW at dst.  tap = 2*block
 * + conv for the 18 fused conv+BN+ReLU stages in state-dict order (0 = unet.inc.double_conv.0 ... 17 =
 * unet.up4.conv.double_conv.3); taps 18..21 = the upsampled + padded half of up1..up4's concat input (`self.up(x1)` +
 * F.pad, unet.py:47-53) where it exists as a tensor (always with the ConvTranspose2d decoder and in BF16X2; for the
 * bilinear decoder only where upsample_kernel materialises it - otherwise FIUNET_ERR_UNSUPPORTED).  out_dims receives
 * {C, H, W} of that activation - C depends on the decoder (the ConvTranspose2d variant is wider at taps 8, 9, 11, 13, 15).  dst_capacity = floats dst can hold; B*C*H*W are written,
 * FIUNET_ERR_INVALID_ARG if it is short.  dst == NULL: dims-only query (nothing is read, workspace may be NULL). */
int fiunet_debug_read_activation(fiunet_ctx* ctx, const void* workspace, int B, int H, int W,
                                 int precision, int tap, float* dst, size_t dst_capacity, int out_dims[3],
                                 void* stream);

/* Measurement hook (bench.py's roofline leg): when enabled, every fiunet_forward records a HIP
 * event on its stream before the first kernel and after each of the 18 conv stages.
 * fiunet_profile_read synchronises on them and returns, per stage, the average duration in
 * ms over the forwards recorded since enable/last read, the stage's algorithmic FLOPs
 * (2*B*H*W*9*Cin*Cout) and the name of the kernel instantiation that ran it
 * (names: 18 strings of name_stride bytes).  Not for use under stream capture. */
int fiunet_profile_enable(fiunet_ctx* ctx, int enable);
int fiunet_profile_read(fiunet_ctx* ctx, int* n_forwards, float* avg_ms, double* flops,
                        char* names, int name_stride);

/* Thread-local description of the last non-OK status. */
const char* fiunet_last_error_string(void);

int fiunet_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FIUNET_H */
