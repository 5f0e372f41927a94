// video.hip -- operations on frame sequences: scene cuts and repeated frames (scene.hip.h), frame-rate conversion
// (retime.hip.h, shutter.hip.h), resizing frame planes (resize.hip.h) and deinterlacing (deinterlace.hip.h).
#include "fiunet_internal.h"
#include "plane_check.h"
#include "scene.hip.h"
#include "retime.hip.h"
#include "shutter.hip.h"
#include "resize.hip.h"
#include "deinterlace.hip.h"
#include "ivtc.hip.h"

using namespace fiunet;

extern "C" {

// ---- scene cuts (csrc/scene.hip.h) -------------------------------------------------------------
constexpr int kMaxGridY = 65535;   // pairs / intervals per launch (grid.y)

extern "C++" {   // (a template inside the extern "C" block)
template <typename T>
static int pair_sad(const T* frames, int n_frames, size_t frame_samples, int64_t* sums, void* stream)
{
    if (!frames || !sums) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (n_frames < 0) return fail(FIUNET_ERR_INVALID_ARG, "n_frames < 0");
    if (n_frames < 2 || frame_samples == 0) return FIUNET_OK;
    // ~4 x 16 B per thread and at most 128 workgroups (= atomics) per pair, as fiunet_psnr_u8
    const unsigned bx = (unsigned)std::min<size_t>((frame_samples * sizeof(T) / 64 + 255) / 256 + 1, 128);
    for (int p0 = 0; p0 < n_frames - 1; p0 += kMaxGridY) {
        const int np = std::min(n_frames - 1 - p0, kMaxGridY);
        hipLaunchKernelGGL(pair_sad_kernel<T>, dim3(bx, (unsigned)np), dim3(kSceneBlock), 0, (hipStream_t)stream,
                           frames + (size_t)p0 * frame_samples, frame_samples,
                           reinterpret_cast<unsigned long long*>(sums + p0));
        HIP_TRY(hipGetLastError());
    }
    return FIUNET_OK;
}
}  // extern "C++"

int fiunet_pair_sad_u8(const uint8_t* frames, int n_frames, size_t frame_samples, int64_t* sums, void* stream)
{
    return pair_sad(frames, n_frames, frame_samples, sums, stream);
}

int fiunet_pair_sad_p10(const uint16_t* frames, int n_frames, size_t frame_samples, int64_t* sums, void* stream)
{
    return pair_sad(frames, n_frames, frame_samples, sums, stream);
}

// repeated frames: the calling conventions of pair_sad
extern "C++" {
template <typename T>
static int pair_peak(const T* frames, int n_frames, size_t frame_samples, uint32_t* peaks, void* stream)
{
    if (!frames || !peaks) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (n_frames < 0) return fail(FIUNET_ERR_INVALID_ARG, "n_frames < 0");
    if (n_frames < 2 || frame_samples == 0) return FIUNET_OK;
    const unsigned bx = (unsigned)std::min<size_t>((frame_samples * sizeof(T) / 64 + 255) / 256 + 1, 128);
    for (int p0 = 0; p0 < n_frames - 1; p0 += kMaxGridY) {
        const int np = std::min(n_frames - 1 - p0, kMaxGridY);
        hipLaunchKernelGGL(pair_peak_kernel<T>, dim3(bx, (unsigned)np), dim3(kSceneBlock), 0, (hipStream_t)stream,
                           frames + (size_t)p0 * frame_samples, frame_samples, peaks + p0);
        HIP_TRY(hipGetLastError());
    }
    return FIUNET_OK;
}
}  // extern "C++"

int fiunet_pair_peak_u8(const uint8_t* frames, int n_frames, size_t frame_samples, uint32_t* peaks, void* stream)
{
    return pair_peak(frames, n_frames, frame_samples, peaks, stream);
}

int fiunet_pair_peak_p10(const uint16_t* frames, int n_frames, size_t frame_samples, uint32_t* peaks, void* stream)
{
    return pair_peak(frames, n_frames, frame_samples, peaks, stream);
}

int fiunet_scene_cuts(const int64_t* sums, int n_frames, size_t count, int bits, double threshold, double* scores,
                      uint8_t* flags, void* stream)
{
    if (!sums || !scores || !flags) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (n_frames < 0) return fail(FIUNET_ERR_INVALID_ARG, "n_frames < 0");
    if (bits != 8 && bits != 10) return fail(FIUNET_ERR_INVALID_ARG, "bits must be 8 or 10");
    if (!(threshold > 0.0 && threshold <= 100.0)) return fail(FIUNET_ERR_INVALID_ARG, "threshold outside (0, 100]");
    if (count == 0) return fail(FIUNET_ERR_INVALID_ARG, "count == 0");
    if (n_frames < 2) return FIUNET_OK;
    const int intervals = n_frames - 1;
    hipLaunchKernelGGL(scene_cuts_kernel, dim3((unsigned)((intervals + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, reinterpret_cast<const long long*>(sums), intervals, (double)count,
                       (double)(1 << bits), threshold, scores, flags);
    HIP_TRY(hipGetLastError());
    return FIUNET_OK;
}

int fiunet_hold_cut_frames(uint8_t* video, int n_frames, size_t frame_bytes, int factor, const uint8_t* flags,
                           void* stream)
{
    if (!video || !flags) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (n_frames < 0) return fail(FIUNET_ERR_INVALID_ARG, "n_frames < 0");
    if (factor < 2 || (factor & (factor - 1)) || factor > (1 << 20))
        return fail(FIUNET_ERR_INVALID_ARG, "factor must be a power of two in [2, 2^20]");
    if (n_frames < 2 || frame_bytes == 0) return FIUNET_OK;
    const unsigned gx = (unsigned)kHoldBlocks * (unsigned)(factor - 1);
    for (int i0 = 0; i0 < n_frames - 1; i0 += kMaxGridY) {
        const int ni = std::min(n_frames - 1 - i0, kMaxGridY);
        hipLaunchKernelGGL(hold_cut_frames_kernel, dim3(gx, (unsigned)ni), dim3(kSceneBlock), 0, (hipStream_t)stream,
                           video + (size_t)i0 * factor * frame_bytes, frame_bytes, factor, flags + i0);
        HIP_TRY(hipGetLastError());
    }
    return FIUNET_OK;
}

// ---- frame-rate conversion (csrc/retime.hip.h) ---------------------------------------------------
extern "C++" {
template <typename T>
static int retime(const T* grid, int n_intervals, size_t frame_samples, int depth, uint64_t first_interval, uint64_t j0,
                  int n_out, uint32_t p, uint32_t q, int mode, const uint8_t* flags, T* out, void* stream)
{
    if (!grid || !out) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (n_intervals < 0 || n_out < 0) return fail(FIUNET_ERR_INVALID_ARG, "negative count");
    if (depth < 1 || depth > 4) return fail(FIUNET_ERR_INVALID_ARG, "depth outside 1..4");
    if (p == 0 || p >= q) return fail(FIUNET_ERR_INVALID_ARG, "need 0 < p < q");
    if (q > kRetimeMaxQ) return fail(FIUNET_ERR_INVALID_ARG, "q above 2^20");
    if (mode != 0 && mode != 1) return fail(FIUNET_ERR_INVALID_ARG, "mode must be 0 (blend) or 1 (nearest)");
    if (n_out == 0) return FIUNET_OK;
    // the first and the last requested frame lie in the grid (the times in between do, being monotonic); in 128 bits,
    // so that the kernel's 64-bit j * p cannot wrap
    const unsigned __int128 t0 = (unsigned __int128)j0 * p, t1 = ((unsigned __int128)j0 + (unsigned)(n_out - 1)) * p;
    if (t1 >> 64) return fail(FIUNET_ERR_INVALID_ARG, "frame index too large");
    const unsigned __int128 end = (unsigned __int128)first_interval + (unsigned)n_intervals;
    if (t0 / q < first_interval) return fail(FIUNET_ERR_INVALID_ARG, "first frame lies before the grid");
    if (t1 / q > end || (t1 / q == end && t1 % q != 0))
        return fail(FIUNET_ERR_INVALID_ARG, "last frame lies behind the grid");
    if (frame_samples == 0) return FIUNET_OK;
    // ~4 x 16 B per thread and at most 128 workgroups per frame, as fiunet_pair_sad_u8
    const unsigned bx = (unsigned)std::min<size_t>((frame_samples * sizeof(T) / 64 + 255) / 256 + 1, 128);
    for (int k0 = 0; k0 < n_out; k0 += kMaxGridY) {
        const int nk = std::min(n_out - k0, kMaxGridY);
        hipLaunchKernelGGL(retime_kernel<T>, dim3(bx, (unsigned)nk), dim3(kRetimeBlock), 0, (hipStream_t)stream, grid,
                           frame_samples, depth, (unsigned long long)first_interval, (unsigned long long)(j0 + k0), p, q,
                           mode, flags, out + (size_t)k0 * frame_samples);
        HIP_TRY(hipGetLastError());
    }
    return FIUNET_OK;
}
}  // extern "C++"

int fiunet_retime_u8(const uint8_t* grid, int n_intervals, size_t frame_samples, int depth, uint64_t first_interval,
                     uint64_t j0, int n_out, uint32_t p, uint32_t q, int mode, const uint8_t* flags, uint8_t* out,
                     void* stream)
{
    return retime(grid, n_intervals, frame_samples, depth, first_interval, j0, n_out, p, q, mode, flags, out, stream);
}

int fiunet_retime_p10(const uint16_t* grid, int n_intervals, size_t frame_samples, int depth, uint64_t first_interval,
                      uint64_t j0, int n_out, uint32_t p, uint32_t q, int mode, const uint8_t* flags, uint16_t* out,
                      void* stream)
{
    return retime(grid, n_intervals, frame_samples, depth, first_interval, j0, n_out, p, q, mode, flags, out, stream);
}

// the table-driven form: every entry is checked here, on the host, before the first launch; the entries
// travel in the kernel's arguments, kRetimeTableMax output frames per launch
static_assert(sizeof(fiunet_retime_entry) == sizeof(RetimeEntry) && sizeof(RetimeEntry) == 12, "entry layout");

extern "C++" {
template <typename T>
static int retime_table(const T* grid, int n_rows, size_t frame_samples, const fiunet_retime_entry* entries, int n_out,
                        T* out, void* stream)
{
    if (!grid || !out) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (n_rows < 0 || n_out < 0) return fail(FIUNET_ERR_INVALID_ARG, "negative count");
    if (n_out == 0) return FIUNET_OK;
    if (!entries) return fail(FIUNET_ERR_INVALID_ARG, "NULL entries");
    for (int k = 0; k < n_out; ++k) {
        const fiunet_retime_entry& e = entries[k];
        if (e.den < 1 || e.den > kRetimeMaxQ) return fail(FIUNET_ERR_INVALID_ARG, "entry: den outside 1..2^20");
        if (e.wn >= e.den) return fail(FIUNET_ERR_INVALID_ARG, "entry: wn >= den");
        if ((uint64_t)e.row >= (uint64_t)n_rows) return fail(FIUNET_ERR_INVALID_ARG, "entry: row outside the grid");
        if (e.wn > 0 && (uint64_t)e.row + 1 >= (uint64_t)n_rows)
            return fail(FIUNET_ERR_INVALID_ARG, "entry: the row after `row` lies outside the grid");
    }
    if (frame_samples == 0) return FIUNET_OK;
    const unsigned bx = (unsigned)std::min<size_t>((frame_samples * sizeof(T) / 64 + 255) / 256 + 1, 128);
    for (int k0 = 0; k0 < n_out; k0 += kRetimeTableMax) {
        const int nk = std::min(n_out - k0, kRetimeTableMax);
        RetimeTable table = {};
        for (int k = 0; k < nk; ++k) table.e[k] = RetimeEntry{entries[k0 + k].row, entries[k0 + k].wn, entries[k0 + k].den};
        hipLaunchKernelGGL(retime_table_kernel<T>, dim3(bx, (unsigned)nk), dim3(kRetimeBlock), 0, (hipStream_t)stream,
                           grid, frame_samples, table, out + (size_t)k0 * frame_samples);
        HIP_TRY(hipGetLastError());
    }
    return FIUNET_OK;
}
}  // extern "C++"

int fiunet_retime_table_u8(const uint8_t* grid, int n_rows, size_t frame_samples, const fiunet_retime_entry* entries,
                           int n_out, uint8_t* out, void* stream)
{
    return retime_table(grid, n_rows, frame_samples, entries, n_out, out, stream);
}

int fiunet_retime_table_p10(const uint16_t* grid, int n_rows, size_t frame_samples, const fiunet_retime_entry* entries,
                            int n_out, uint16_t* out, void* stream)
{
    return retime_table(grid, n_rows, frame_samples, entries, n_out, out, stream);
}

// ---- a synthesized shutter (csrc/shutter.hip.h) ---------------------------------------------------------
// `entries` is a run of 32-bit words, per output frame: first_row, n_taps, then n_taps weights.  Every entry is checked
// here, on the host, before the first launch (n_taps before its weights are read); the entries travel in the kernel's
// arguments, as many frames per launch as ShutterArgs holds.
extern "C++" {
template <typename T>
static int shutter(const T* grid, int n_rows, size_t frame_samples, const uint32_t* entries, int n_out, T* out, void* stream)
{
    if (!grid || !out) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (n_rows < 0 || n_out < 0) return fail(FIUNET_ERR_INVALID_ARG, "negative count");
    if (n_out == 0) return FIUNET_OK;
    if (!entries) return fail(FIUNET_ERR_INVALID_ARG, "NULL entries");
    const uint32_t* e = entries;
    for (int k = 0; k < n_out; ++k) {
        const uint32_t row = e[0], taps = e[1];
        if (taps < 1 || taps > (uint32_t)kShutterMaxTaps) return fail(FIUNET_ERR_INVALID_ARG, "entry: n_taps outside 1..48");
        if ((uint64_t)row + taps > (uint64_t)n_rows) return fail(FIUNET_ERR_INVALID_ARG, "entry: a tap row outside the grid");
        uint64_t sum = 0;
        for (uint32_t t = 0; t < taps; ++t) sum += e[2 + t];
        if (sum != kShutterOne) return fail(FIUNET_ERR_INVALID_ARG, "entry: the weights do not sum to 2^20");
        e += 2 + taps;
    }
    if (frame_samples == 0) return FIUNET_OK;
    // ~2 x 16 B per thread and at most 256 workgroups per frame
    const unsigned bx = (unsigned)std::min<size_t>((frame_samples * sizeof(T) / 32 + 255) / 256 + 1, 256);
    e = entries;
    for (int k0 = 0; k0 < n_out;) {
        ShutterArgs args = {};
        int nk = 0, nw = 0;
        const int most = std::min(n_out - k0, kShutterMaxFrames);   // (one frame always fits: n_taps <= 48)
        while (nk < most && nw + (int)e[1] <= kShutterMaxWeights) {
            uint32_t row = e[0], taps = e[1];
            const uint32_t* w = e + 2;
            for (uint32_t t = 0; t < taps; ++t)
                if (w[t] == kShutterOne) { row += t, w += t, taps = 1; break; }   // one live tap: the kernel's copy
            args.row[nk] = row, args.off[nk] = (uint16_t)nw, args.taps[nk] = (uint16_t)taps;
            for (uint32_t t = 0; t < taps; ++t) args.w[nw + t] = w[t];
            nw += (int)taps, ++nk;
            e += 2 + e[1];
        }
        hipLaunchKernelGGL(shutter_kernel<T>, dim3(bx, (unsigned)nk), dim3(kShutterBlock), 0, (hipStream_t)stream, grid,
                           frame_samples, args, out + (size_t)k0 * frame_samples);
        HIP_TRY(hipGetLastError());
        k0 += nk;
    }
    return FIUNET_OK;
}
}  // extern "C++"

int fiunet_shutter_u8(const uint8_t* grid, int n_rows, size_t frame_samples, const uint32_t* entries, int n_out,
                      uint8_t* out, void* stream)
{
    return shutter(grid, n_rows, frame_samples, entries, n_out, out, stream);
}

int fiunet_shutter_p10(const uint16_t* grid, int n_rows, size_t frame_samples, const uint32_t* entries, int n_out,
                       uint16_t* out, void* stream)
{
    return shutter(grid, n_rows, frame_samples, entries, n_out, out, stream);
}

// ---- resizing frame planes (csrc/resize.hip.h) ------------------------------------------------------
extern "C++" {
template <typename T>
static int resize_planes(const T* src, const fiunet_resize_plane* sp, T* dst, const fiunet_resize_plane* dp,
                         int n_planes, int n_frames, void* stream)
{
    if (!src || !dst || !sp || !dp) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (((uintptr_t)src | (uintptr_t)dst) % sizeof(T)) return fail(FIUNET_ERR_INVALID_ARG, "misaligned pointer");
    if (n_planes < 1 || n_planes > kResizeMaxPlanes) return fail(FIUNET_ERR_INVALID_ARG, "n_planes must be 1..4");
    if (n_frames < 0) return fail(FIUNET_ERR_INVALID_ARG, "n_frames < 0");
    constexpr int V = ResizeSample<T>::kVec;
    // the filter is the destination planes' (they agree); a source plane carries 0
    const int filter = dp[0].filter;
    for (int i = 0; i < n_planes; ++i) {
        if (sp[i].filter != 0) return fail(FIUNET_ERR_INVALID_ARG, "a source plane's filter must be 0");
        if (dp[i].filter != FIUNET_RESIZE_LINEAR && dp[i].filter != FIUNET_RESIZE_AREA)
            return fail(FIUNET_ERR_INVALID_ARG, "a destination plane's filter must be FIUNET_RESIZE_LINEAR or FIUNET_RESIZE_AREA");
        if (dp[i].filter != filter) return fail(FIUNET_ERR_INVALID_ARG, "the destination planes of one call must name one filter");
    }
    // the planes of a launch: the linear kernel's (under the area filter, the planes of equal size: its copy) and the
    // area kernel's
    ResizeArgs base[2] = {};
    int count[2] = {0, 0};
    unsigned long long per_frame_max = 0;
    // the bytes [lo, hi) of n_frames frames of all source planes [0] and of all destination planes [1]
    uintptr_t lo[2] = {UINTPTR_MAX, UINTPTR_MAX}, hi[2] = {0, 0};
    for (int i = 0; i < n_planes; ++i) {
        for (int d = 0; d < 2; ++d) {
            const fiunet_resize_plane& p = d ? dp[i] : sp[i];
            if (const char* why = plane_check(p, kResizeMaxSize)) return fail(FIUNET_ERR_INVALID_ARG, why);
            if (n_frames == 0) continue;
            uintptr_t p0, p1;
            if (!plane_range(d ? (const void*)dst : src, sizeof(T), p, n_frames, &p0, &p1))
                return fail(FIUNET_ERR_INVALID_ARG, "a plane's frame stride is too large");
            lo[d] = std::min(lo[d], p0), hi[d] = std::max(hi[d], p1);
        }
        const bool equal = sp[i].h == dp[i].h && sp[i].w == dp[i].w;
        if (filter == FIUNET_RESIZE_AREA) {
            if (dp[i].w > sp[i].w || dp[i].h > sp[i].h)
                return fail(FIUNET_ERR_INVALID_ARG, "the area filter only down-scales a plane: use the linear filter to enlarge");
            if ((long long)sp[i].w > (long long)kResizeAreaMaxRatio * dp[i].w ||
                (long long)sp[i].h > (long long)kResizeAreaMaxRatio * dp[i].h)
                return fail(FIUNET_ERR_UNSUPPORTED, "the area filter covers ratios up to 64 on either axis");
        }
        const int which = filter == FIUNET_RESIZE_AREA && !equal ? 1 : 0;
        ResizePlane& P = base[which].p[count[which]++];
        P.src_off = sp[i].offset, P.src_pitch = sp[i].pitch, P.src_fs = sp[i].frame_stride;
        P.dst_off = dp[i].offset, P.dst_pitch = dp[i].pitch, P.dst_fs = dp[i].frame_stride;
        P.sh = sp[i].h, P.sw = sp[i].w, P.dh = dp[i].h, P.dw = dp[i].w;
        P.sstep = sp[i].step, P.dstep = dp[i].step;
        P.sx = (double)P.sw / (double)P.dw, P.sy = (double)P.sh / (double)P.dh;
        P.chunks = (unsigned)((P.dw + V - 1) / V) + (P.dstep == 1 ? 1u : 0u);
        P.inv_dw = 1.0 / (double)P.dw, P.inv_dh = 1.0 / (double)P.dh, P.inv_chunks = 1.0 / (double)P.chunks;
        const unsigned long long per_frame = (unsigned long long)P.dh * P.chunks;
        if (per_frame >= (1ull << 31)) return fail(FIUNET_ERR_UNSUPPORTED, "a destination plane of 2^31 or more store chunks");
        per_frame_max = std::max(per_frame_max, per_frame);
    }
    if (n_frames == 0) return FIUNET_OK;
    if (ranges_overlap(lo[0], hi[0], lo[1], hi[1])) return fail(FIUNET_ERR_INVALID_ARG, "source and destination overlap");
    // frames per launch: every plane's item count stays below 2^31
    const int batch = (int)std::min<unsigned long long>(((1ull << 31) - 1) / per_frame_max, (unsigned long long)n_frames);
    for (int f0 = 0; f0 < n_frames; f0 += batch) {
        const int nf = std::min(batch, n_frames - f0);
        for (int which = 0; which < 2; ++which) {
            if (!count[which]) continue;
            ResizeArgs args = base[which];
            unsigned items_max = 0;
            for (int i = 0; i < count[which]; ++i) {
                ResizePlane& P = args.p[i];
                P.src_off += (size_t)f0 * P.src_fs, P.dst_off += (size_t)f0 * P.dst_fs;
                P.items = (unsigned)nf * (unsigned)P.dh * P.chunks;
                items_max = std::max(items_max, P.items);
            }
            if (which == 0) {
                // one item per thread up to 8192 workgroups (32 per CU), a grid-stride loop beyond
                const unsigned bx = std::min((items_max + kResizeBlock - 1) / kResizeBlock, 8192u);
                hipLaunchKernelGGL(resize_planes_kernel<T>, dim3(bx, (unsigned)count[0]), dim3(kResizeBlock), 0,
                                   (hipStream_t)stream, src, dst, args);
            } else {
                // kVec lanes per item: kResizeBlock / kVec items per workgroup, up to 65536 workgroups
                constexpr unsigned per_wg = kResizeBlock / V;
                const unsigned bx = std::min((items_max + per_wg - 1) / per_wg, 65536u);
                hipLaunchKernelGGL(resize_area_kernel<T>, dim3(bx, (unsigned)count[1]), dim3(kResizeBlock), 0,
                                   (hipStream_t)stream, src, dst, args);
            }
            HIP_TRY(hipGetLastError());
        }
    }
    return FIUNET_OK;
}
}  // extern "C++"

int fiunet_resize_planes_u8(const uint8_t* src, const fiunet_resize_plane* src_planes, uint8_t* dst,
                            const fiunet_resize_plane* dst_planes, int n_planes, int n_frames, void* stream)
{
    return resize_planes(src, src_planes, dst, dst_planes, n_planes, n_frames, stream);
}

int fiunet_resize_planes_p10(const uint16_t* src, const fiunet_resize_plane* src_planes, uint16_t* dst,
                             const fiunet_resize_plane* dst_planes, int n_planes, int n_frames, void* stream)
{
    return resize_planes(src, src_planes, dst, dst_planes, n_planes, n_frames, stream);
}

// ---- deinterlacing (csrc/deinterlace.hip.h) -------------------------------------------------------------
extern "C++" {
template <typename T, int V>
static void deinterlace_launch(const T* src, T* dst, const DeintPlane& P, dim3 grid, int n_src, int first, int bff, int field,
                               int method, bool spatial, hipStream_t stream)
{
    if (method == FIUNET_DEINT_BOB)
        hipLaunchKernelGGL((deinterlace_kernel<T, V, 0, false>), grid, dim3(kDeintBlock), 0, stream, src, dst, P, n_src, first, bff, field);
    else if (spatial)
        hipLaunchKernelGGL((deinterlace_kernel<T, V, 1, true>), grid, dim3(kDeintBlock), 0, stream, src, dst, P, n_src, first, bff, field);
    else
        hipLaunchKernelGGL((deinterlace_kernel<T, V, 1, false>), grid, dim3(kDeintBlock), 0, stream, src, dst, P, n_src, first, bff, field);
}

template <typename T>
static int deinterlace(const T* src, int n_src, const fiunet_resize_plane* sp, T* dst, const fiunet_resize_plane* dp,
                       int n_planes, int first, int n_frames, int order, int rate, int method_flags, void* stream)
{
    if (!src || !dst || !sp || !dp) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (((uintptr_t)src | (uintptr_t)dst) % sizeof(T)) return fail(FIUNET_ERR_INVALID_ARG, "misaligned pointer");
    if (n_planes < 1 || n_planes > kResizeMaxPlanes) return fail(FIUNET_ERR_INVALID_ARG, "n_planes must be 1..4");
    if (order != FIUNET_DEINT_TFF && order != FIUNET_DEINT_BFF) return fail(FIUNET_ERR_INVALID_ARG, "order must be FIUNET_DEINT_TFF or FIUNET_DEINT_BFF");
    if (rate != FIUNET_DEINT_FIELD_RATE && rate != FIUNET_DEINT_FRAME_RATE)
        return fail(FIUNET_ERR_INVALID_ARG, "rate must be FIUNET_DEINT_FIELD_RATE or FIUNET_DEINT_FRAME_RATE");
    const int method = method_flags & 0xff;
    if ((method != FIUNET_DEINT_ADAPTIVE && method != FIUNET_DEINT_BOB) || (method_flags & ~(0xff | FIUNET_DEINT_NO_SPATIAL_CHECK)))
        return fail(FIUNET_ERR_INVALID_ARG, "method_flags: FIUNET_DEINT_ADAPTIVE or FIUNET_DEINT_BOB, with or without FIUNET_DEINT_NO_SPATIAL_CHECK");
    if (n_src < 0 || first < 0 || n_frames < 0 || first > n_src || n_frames > n_src - first)
        return fail(FIUNET_ERR_INVALID_ARG, "first and n_frames must name frames of the window of n_src");
    const int per = rate == FIUNET_DEINT_FIELD_RATE ? 2 : 1;
    if (n_frames > kDeintMaxOut / per) return fail(FIUNET_ERR_INVALID_ARG, "more than 65535 output frames in one call");
    const int n_out = n_frames * per;
    uintptr_t lo[2] = {UINTPTR_MAX, UINTPTR_MAX}, hi[2] = {0, 0};   // [0]: n_src source frames, [1]: n_out of dst
    for (int i = 0; i < n_planes; ++i) {
        for (int d = 0; d < 2; ++d) {
            const fiunet_resize_plane& p = d ? dp[i] : sp[i];
            if (const char* why = plane_check(p, kResizeMaxSize)) return fail(FIUNET_ERR_INVALID_ARG, why);
            if (p.filter != 0) return fail(FIUNET_ERR_INVALID_ARG, "a plane's filter must be 0");
            if (p.h < 2) return fail(FIUNET_ERR_INVALID_ARG, "a plane needs two rows or more: h < 2");
            const int n = d ? n_out : n_src;
            if (n == 0) continue;
            uintptr_t p0, p1;
            if (!plane_range(d ? (const void*)dst : src, sizeof(T), p, n, &p0, &p1))
                return fail(FIUNET_ERR_INVALID_ARG, "a plane's frame stride is too large");
            lo[d] = std::min(lo[d], p0), hi[d] = std::max(hi[d], p1);
        }
        if (sp[i].h != dp[i].h || sp[i].w != dp[i].w)
            return fail(FIUNET_ERR_INVALID_ARG, "a source plane and its destination plane differ in size");
    }
    if (n_frames == 0) return FIUNET_OK;
    if (ranges_overlap(lo[0], hi[0], lo[1], hi[1])) return fail(FIUNET_ERR_INVALID_ARG, "source and destination overlap");
    const bool spatial = !(method_flags & FIUNET_DEINT_NO_SPATIAL_CHECK);
    constexpr int V = 16 / (int)sizeof(T);
    for (int i = 0; i < n_planes; ++i) {
        const DeintPlane P = {sp[i].offset, sp[i].pitch, sp[i].frame_stride, dp[i].offset, dp[i].pitch, dp[i].frame_stride,
                              sp[i].h, sp[i].w, sp[i].step, dp[i].step};
        // the vector path: step 1 and every row of every frame 16-byte aligned, on both sides
        const size_t bytes = ((uintptr_t)(src + P.src_off) | (uintptr_t)(dst + P.dst_off) |
                              (P.src_pitch | P.src_fs | P.dst_pitch | P.dst_fs) * sizeof(T));
        const bool vec = P.sstep == 1 && P.dstep == 1 && bytes % 16 == 0;
        const unsigned per_lane = vec ? V : 1;
        const unsigned lanes = ((unsigned)P.w + per_lane - 1) / per_lane;
        const dim3 grid((lanes + 63) / 64, std::min(((unsigned)(P.h + 1) / 2 + 3) / 4, kDeintMaxRowGroups), (unsigned)n_out);
        if (vec) deinterlace_launch<T, V>(src, dst, P, grid, n_src, first, order == FIUNET_DEINT_BFF, per == 2, method, spatial, (hipStream_t)stream);
        else deinterlace_launch<T, 1>(src, dst, P, grid, n_src, first, order == FIUNET_DEINT_BFF, per == 2, method, spatial, (hipStream_t)stream);
        HIP_TRY(hipGetLastError());
    }
    return FIUNET_OK;
}
}  // extern "C++"

int fiunet_deinterlace_u8(const uint8_t* src, int n_src, const fiunet_resize_plane* src_planes, uint8_t* dst,
                          const fiunet_resize_plane* dst_planes, int n_planes, int first, int n_frames, int order, int rate,
                          int method_flags, void* stream)
{
    return deinterlace(src, n_src, src_planes, dst, dst_planes, n_planes, first, n_frames, order, rate, method_flags, stream);
}

int fiunet_deinterlace_p10(const uint16_t* src, int n_src, const fiunet_resize_plane* src_planes, uint16_t* dst,
                           const fiunet_resize_plane* dst_planes, int n_planes, int first, int n_frames, int order, int rate,
                           int method_flags, void* stream)
{
    return deinterlace(src, n_src, src_planes, dst, dst_planes, n_planes, first, n_frames, order, rate, method_flags, stream);
}

// ---- inverse telecine (csrc/ivtc.hip.h) -----------------------------------------------------------------
static_assert(sizeof(fiunet_weave_entry) == 8, "entry layout");

extern "C++" {
template <typename T>
static int field_match(const T* src, int n_src, const fiunet_resize_plane* plane, int first, int n_frames, int order,
                       int threshold, uint32_t* scores, void* stream)
{
    if (!src || !plane || !scores) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if ((uintptr_t)src % sizeof(T) || (uintptr_t)scores % sizeof(uint32_t)) return fail(FIUNET_ERR_INVALID_ARG, "misaligned pointer");
    if (order != FIUNET_DEINT_TFF && order != FIUNET_DEINT_BFF) return fail(FIUNET_ERR_INVALID_ARG, "order must be FIUNET_DEINT_TFF or FIUNET_DEINT_BFF");
    if (threshold < 0 || threshold > kMatchMaxThreshold) return fail(FIUNET_ERR_INVALID_ARG, "threshold outside 0..1023");
    if (n_src < 0 || first < 0 || n_frames < 0 || first > n_src || n_frames > n_src - first)
        return fail(FIUNET_ERR_INVALID_ARG, "first and n_frames must name frames of the window of n_src");
    if (n_frames > kMatchMaxFrames) return fail(FIUNET_ERR_INVALID_ARG, "more than 65535 frames in one call");
    if (const char* why = plane_check(*plane, kResizeMaxSize)) return fail(FIUNET_ERR_INVALID_ARG, why);
    if (plane->filter != 0) return fail(FIUNET_ERR_INVALID_ARG, "a plane's filter must be 0");
    if (plane->h < 3) return fail(FIUNET_ERR_INVALID_ARG, "the comb score needs three rows or more: h < 3");
    if (n_frames == 0) return FIUNET_OK;
    uintptr_t s0, s1;
    if (!plane_range(src, sizeof(T), *plane, n_src, &s0, &s1)) return fail(FIUNET_ERR_INVALID_ARG, "a plane's frame stride is too large");
    const uintptr_t d0 = (uintptr_t)scores;
    if (ranges_overlap(s0, s1, d0, d0 + (size_t)n_frames * 3 * sizeof(uint32_t)))
        return fail(FIUNET_ERR_INVALID_ARG, "source and destination overlap");
    const MatchPlane P = {plane->offset, plane->pitch, plane->frame_stride, plane->h, plane->w, plane->step};
    constexpr int V = 16 / (int)sizeof(T);
    // the vector path: step 1 and every row of every frame 16-byte aligned
    const bool vec = P.step == 1 && ((uintptr_t)(src + P.off) | (P.pitch | P.fs) * sizeof(T)) % 16 == 0;
    const unsigned per_lane = vec ? V : 1;
    const unsigned lanes = ((unsigned)P.w + per_lane - 1) / per_lane;
    const unsigned block_rows = ((unsigned)P.h + kMatchRows - 1) / kMatchRows;
    const dim3 grid((lanes + 63) / 64, std::min((block_rows + 3) / 4, kMatchMaxRowGroups), (unsigned)n_frames);
    const int keep = order == FIUNET_DEINT_BFF, t2 = threshold * threshold;
    if (vec) hipLaunchKernelGGL((field_match_kernel<T, V>), grid, dim3(kMatchBlock), 0, (hipStream_t)stream, src, P, n_src, first, keep, t2, scores);
    else hipLaunchKernelGGL((field_match_kernel<T, 1>), grid, dim3(kMatchBlock), 0, (hipStream_t)stream, src, P, n_src, first, keep, t2, scores);
    HIP_TRY(hipGetLastError());
    return FIUNET_OK;
}

template <typename T>
static int field_weave(const T* src, int n_src, const fiunet_resize_plane* sp, T* dst, const fiunet_resize_plane* dp, int n_planes,
                       const fiunet_weave_entry* entries, int n_out, int parity, void* stream)
{
    if (!src || !dst || !sp || !dp) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (((uintptr_t)src | (uintptr_t)dst) % sizeof(T)) return fail(FIUNET_ERR_INVALID_ARG, "misaligned pointer");
    if (n_planes < 1 || n_planes > kWeaveMaxPlanes) return fail(FIUNET_ERR_INVALID_ARG, "n_planes must be 1..4");
    if (parity != 0 && parity != 1) return fail(FIUNET_ERR_INVALID_ARG, "parity must be 0 (even rows) or 1 (odd rows)");
    if (n_src < 0 || n_out < 0) return fail(FIUNET_ERR_INVALID_ARG, "negative count");
    if (n_out > kWeaveMaxOut) return fail(FIUNET_ERR_INVALID_ARG, "more than 65535 output frames in one call");
    if (n_out > 0 && !entries) return fail(FIUNET_ERR_INVALID_ARG, "NULL entries");
    for (int k = 0; k < n_out; ++k)
        if (std::max(entries[k].keep, entries[k].other) >= (uint32_t)n_src)
            return fail(FIUNET_ERR_INVALID_ARG, "entry: a frame outside the window of n_src");
    uintptr_t lo[2] = {UINTPTR_MAX, UINTPTR_MAX}, hi[2] = {0, 0};   // [0]: n_src source frames, [1]: n_out of dst
    WeaveArgs base = {};
    int rows_max = 0;
    for (int i = 0; i < n_planes; ++i) {
        for (int d = 0; d < 2; ++d) {
            const fiunet_resize_plane& p = d ? dp[i] : sp[i];
            if (const char* why = plane_check(p, kResizeMaxSize)) return fail(FIUNET_ERR_INVALID_ARG, why);
            if (p.filter != 0) return fail(FIUNET_ERR_INVALID_ARG, "a plane's filter must be 0");
            if (p.h < 2) return fail(FIUNET_ERR_INVALID_ARG, "a plane needs two rows or more: h < 2");
            const int n = d ? n_out : n_src;
            if (n == 0) continue;
            uintptr_t p0, p1;
            if (!plane_range(d ? (const void*)dst : src, sizeof(T), p, n, &p0, &p1))
                return fail(FIUNET_ERR_INVALID_ARG, "a plane's frame stride is too large");
            lo[d] = std::min(lo[d], p0), hi[d] = std::max(hi[d], p1);
        }
        if (sp[i].h != dp[i].h || sp[i].w != dp[i].w)
            return fail(FIUNET_ERR_INVALID_ARG, "a source plane and its destination plane differ in size");
        WeavePlane& P = base.p[i];
        P = {sp[i].offset, sp[i].pitch, sp[i].frame_stride, dp[i].offset, dp[i].pitch, dp[i].frame_stride,
             sp[i].h, sp[i].w, sp[i].step, dp[i].step, 0};
        const size_t bytes = ((uintptr_t)(src + P.src_off) | (uintptr_t)(dst + P.dst_off) |
                              (P.src_pitch | P.src_fs | P.dst_pitch | P.dst_fs) * sizeof(T));
        P.vec = P.sstep == 1 && P.dstep == 1 && bytes % 16 == 0;
        rows_max = std::max(rows_max, P.h);
    }
    if (n_out == 0) return FIUNET_OK;
    if (ranges_overlap(lo[0], hi[0], lo[1], hi[1])) return fail(FIUNET_ERR_INVALID_ARG, "source and destination overlap");
    const unsigned gx = std::min(((unsigned)rows_max + 3) / 4, kWeaveMaxRowGroups);
    for (int k0 = 0; k0 < n_out; k0 += kWeaveMax) {
        const int nk = std::min(n_out - k0, kWeaveMax);
        WeaveArgs args = base;
        for (int i = 0; i < n_planes; ++i) args.p[i].dst_off += (size_t)k0 * args.p[i].dst_fs;
        for (int k = 0; k < nk; ++k) args.keep[k] = entries[k0 + k].keep, args.other[k] = entries[k0 + k].other;
        hipLaunchKernelGGL(field_weave_kernel<T>, dim3(gx, (unsigned)n_planes, (unsigned)nk), dim3(kWeaveBlock), 0,
                           (hipStream_t)stream, src, dst, args, parity);
        HIP_TRY(hipGetLastError());
    }
    return FIUNET_OK;
}
}  // extern "C++"

int fiunet_field_match_u8(const uint8_t* src, int n_src, const fiunet_resize_plane* plane, int first, int n_frames, int order,
                          int threshold, uint32_t* scores, void* stream)
{
    return field_match(src, n_src, plane, first, n_frames, order, threshold, scores, stream);
}

int fiunet_field_match_p10(const uint16_t* src, int n_src, const fiunet_resize_plane* plane, int first, int n_frames, int order,
                           int threshold, uint32_t* scores, void* stream)
{
    return field_match(src, n_src, plane, first, n_frames, order, threshold, scores, stream);
}

int fiunet_field_weave_u8(const uint8_t* src, int n_src, const fiunet_resize_plane* src_planes, uint8_t* dst,
                          const fiunet_resize_plane* dst_planes, int n_planes, const fiunet_weave_entry* entries, int n_out,
                          int parity, void* stream)
{
    return field_weave(src, n_src, src_planes, dst, dst_planes, n_planes, entries, n_out, parity, stream);
}

int fiunet_field_weave_p10(const uint16_t* src, int n_src, const fiunet_resize_plane* src_planes, uint16_t* dst,
                           const fiunet_resize_plane* dst_planes, int n_planes, const fiunet_weave_entry* entries, int n_out,
                           int parity, void* stream)
{
    return field_weave(src, n_src, src_planes, dst, dst_planes, n_planes, entries, n_out, parity, stream);
}

}  // extern "C"
