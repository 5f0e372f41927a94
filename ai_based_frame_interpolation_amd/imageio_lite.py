"""Image file I/O for the inference helpers without OpenCV / imageio (neither is in this image).

The reference reads its frames with `cv2.imread(path, cv2.IMREAD_GRAYSCALE)`, resizes them with
`cv2.resize(image, (256, 256))` and writes results with `cv2.imwrite`
(/root/reference/model/inference.py:23,29,251,284).  This module is the host-side stand-in:

  read_gray(path)            PNG (8/16-bit gray, gray+alpha, RGB, RGBA, palette; non-interlaced), BMP
                             (24/32-bit and 8-bit palette), binary PGM/PPM, `.npy`; colour images are
                             converted with OpenCV's BGR2GRAY weights in its fixed-point form.
  resize_linear_u8(img, wh)  cv2.resize's INTER_LINEAR for uint8: half-pixel centres, edge clamp,
                             11-bit fixed-point coefficients and its two-stage rounding.
  resize_area(img, wh, bits) the device resize's area filter (down-scaling, integers, exact): the host
                             statement of csrc/resize.hip.h's resize_area_kernel.
  write_png(path, img)       8-bit gray or RGB PNG.

Restated from OpenCV's published implementation (imgproc/resize.cpp `resizeGeneric_` with
`HResizeLinear` / `VResizeLinear<uchar,int,short>`, `INTER_RESIZE_COEF_BITS = 11`; color.cpp RGB2Gray
with `yuv_shift = 14` coefficients 4899 / 9617 / 1868).  OpenCV is not installed, so these are
**unpinned against cv2 itself**; the tests pin them to their own definition (identity at equal size,
exact values on hand-computed cases, PNG round trips).  Host glue, not part of the device hot path:
if `cv2` is importable the callers use it instead.
"""
from __future__ import annotations

import os
import struct
import zlib

import numpy as np

_PNG_SIG = b"\x89PNG\r\n\x1a\n"


def _to_gray(rgb: np.ndarray) -> np.ndarray:
    """OpenCV RGB2GRAY on uint8: (R*4899 + G*9617 + B*1868 + 8192) >> 14."""
    r, g, b = (rgb[..., i].astype(np.int32) for i in range(3))
    return ((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14).astype(np.uint8)


def _unfilter(raw: bytes, height: int, stride: int, bpp: int) -> np.ndarray:
    out = np.zeros((height, stride), dtype=np.uint8)
    prev = np.zeros(stride, dtype=np.int32)
    pos = 0
    for y in range(height):
        ft = raw[pos]
        line = np.frombuffer(raw, dtype=np.uint8, count=stride, offset=pos + 1).astype(np.int32)
        pos += stride + 1
        if ft == 0:
            cur = line
        elif ft == 2:  # Up
            cur = (line + prev) & 255
        elif ft == 1:  # Sub: running sum per byte lane
            cur = line.copy()
            for c in range(bpp):
                cur[c::bpp] = np.cumsum(line[c::bpp]) & 255
        else:  # Average / Paeth need the already reconstructed left neighbour: byte-serial
            cur = np.zeros(stride, dtype=np.int32)
            ln, pv = line.tolist(), prev.tolist()
            res = [0] * stride
            for i in range(stride):
                a = res[i - bpp] if i >= bpp else 0
                b = pv[i]
                if ft == 3:
                    res[i] = (ln[i] + ((a + b) >> 1)) & 255
                elif ft == 4:
                    c = pv[i - bpp] if i >= bpp else 0
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pr = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                    res[i] = (ln[i] + pr) & 255
                else:
                    raise ValueError(f"bad PNG filter type {ft}")
            cur = np.asarray(res, dtype=np.int32)
        out[y] = cur
        prev = cur
    return out


def read_png(path: str) -> np.ndarray:
    """-> uint8 [H,W] (gray) or [H,W,3] (RGB; alpha dropped, palette expanded)."""
    data = open(path, "rb").read()
    if data[:8] != _PNG_SIG:
        raise ValueError("not a PNG file")
    pos, idat, plte = 8, [], None
    w = h = depth = ctype = interlace = None
    while pos < len(data):
        ln, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + ln]
        pos += 12 + ln
        if tag == b"IHDR":
            w, h, depth, ctype, _, _, interlace = struct.unpack(">IIBBBBB", body)
        elif tag == b"PLTE":
            plte = np.frombuffer(body, dtype=np.uint8).reshape(-1, 3)
        elif tag == b"IDAT":
            idat.append(body)
        elif tag == b"IEND":
            break
    if interlace:
        raise ValueError("interlaced PNG is not supported")
    nch = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[ctype]
    if depth not in (8, 16) or (ctype == 3 and depth != 8):
        raise ValueError(f"PNG bit depth {depth} / colour type {ctype} is not supported")
    bps = depth // 8
    px = _unfilter(zlib.decompress(b"".join(idat)), h, w * nch * bps, nch * bps).reshape(h, w, nch, bps)
    px = px[..., 0]  # 16-bit: keep the high byte (cv2.imread without IMREAD_ANYDEPTH also narrows to 8 bits)
    if ctype == 3:
        return plte[px[..., 0]]
    if ctype in (0, 4):
        return np.ascontiguousarray(px[..., 0])
    return np.ascontiguousarray(px[..., :3])


def read_bmp(path: str) -> np.ndarray:
    data = open(path, "rb").read()
    if data[:2] != b"BM":
        raise ValueError("not a BMP file")
    off = struct.unpack("<I", data[10:14])[0]
    hdr, w, h, _, bpp, comp = struct.unpack("<IiiHHI", data[14:34])
    if comp not in (0, 3) or bpp not in (8, 24, 32):
        raise ValueError("compressed / unusual BMP is not supported")
    flip = h > 0
    h = abs(h)
    stride = ((w * bpp + 31) // 32) * 4
    rows = np.frombuffer(data, dtype=np.uint8, count=stride * h, offset=off).reshape(h, stride)
    if flip:
        rows = rows[::-1]
    if bpp == 8:
        pal = np.frombuffer(data, dtype=np.uint8, count=256 * 4, offset=14 + hdr).reshape(256, 4)[:, 2::-1]
        return np.ascontiguousarray(pal[rows[:, :w]])
    px = rows[:, :w * (bpp // 8)].reshape(h, w, bpp // 8)
    return np.ascontiguousarray(px[..., 2::-1])  # BGR(A) -> RGB


def _read_pnm(path: str) -> np.ndarray:
    data = open(path, "rb").read()
    tok, pos = [], 0
    while len(tok) < 4:  # magic, width, height, maxval
        while data[pos:pos + 1].isspace():
            pos += 1
        if data[pos:pos + 1] == b"#":
            pos = data.index(b"\n", pos) + 1
            continue
        end = pos
        while not data[end:end + 1].isspace():
            end += 1
        tok.append(data[pos:end]); pos = end
    pos += 1
    w, h = int(tok[1]), int(tok[2])
    ch = 3 if tok[0] == b"P6" else 1
    img = np.frombuffer(data, dtype=np.uint8, count=w * h * ch, offset=pos).reshape(h, w, ch)
    return img[..., 0] if ch == 1 else img


def read_gray(path: str):
    """cv2.imread(path, IMREAD_GRAYSCALE) for the formats above; None if the format is unknown."""
    ext = path.lower().rsplit(".", 1)[-1] if "." in path else ""
    if ext == "npy":
        img = np.load(path)
    elif ext == "png":
        img = read_png(path)
    elif ext == "bmp":
        img = read_bmp(path)
    elif ext in ("pgm", "ppm", "pnm"):
        img = _read_pnm(path)
    else:
        return None
    if img.ndim == 3:
        img = _to_gray(np.clip(img[..., :3], 0, 255).astype(np.uint8))
    return np.clip(img, 0, 255).astype(np.uint8)


def resize_linear_u8(img: np.ndarray, target_size) -> np.ndarray:
    """cv2.resize(img, (W, H)) with the default INTER_LINEAR on a uint8 [H,W] image."""
    tw, th = int(target_size[0]), int(target_size[1])
    sh, sw = img.shape[:2]
    if (sh, sw) == (th, tw):
        return img
    bits = 11
    one = 1 << bits

    def axis(dst_n, src_n):
        scale = src_n / dst_n
        f = ((np.arange(dst_n, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)  # fx is a float
        i0 = np.floor(f).astype(np.int64)
        frac = f - i0.astype(np.float32)
        lo = i0 < 0
        frac[lo] = 0.0
        i0[lo] = 0
        hi = i0 >= src_n - 1
        frac[hi] = 0.0
        i0[hi] = src_n - 1
        i1 = np.minimum(i0 + 1, src_n - 1)
        # saturate_cast<short>(cvRound(w * 2048)): round half to even, like cvRound
        c1 = np.rint(frac.astype(np.float64) * one).astype(np.int64)
        c0 = np.rint((1.0 - frac).astype(np.float64) * one).astype(np.int64)
        return i0, i1, c0, c1

    x0, x1, a0, a1 = axis(tw, sw)
    y0, y1, b0, b1 = axis(th, sh)
    src = img.astype(np.int64)
    rows = src[:, x0] * a0 + src[:, x1] * a1                  # HResizeLinear: int, scaled by 2^11
    r0, r1 = rows[y0], rows[y1]
    # VResizeLinear<uchar,int,short>: ((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2
    out = (((b0[:, None] * (r0 >> 4)) >> 16) + ((b1[:, None] * (r1 >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


AREA_MAX_RATIO = 64   # csrc/resize.hip.h kResizeAreaMaxRatio: the device kernel's limit (the host statement has none)


def check_area(sh: int, sw: int, th: int, tw: int, max_ratio: int | None = None) -> None:
    """The refusals of the area filter for one sh x sw plane resized to th x tw (ValueError): a plane that grows, and,
    with max_ratio (the device's AREA_MAX_RATIO), one that shrinks more than that on either axis."""
    if tw > sw or th > sh:
        raise ValueError(f"the area filter only down-scales: {sw}x{sh} -> {tw}x{th} enlarges a plane; use the linear filter")
    if max_ratio is not None and (sw > max_ratio * tw or sh > max_ratio * th):
        raise ValueError(f"the device's area filter covers ratios up to {max_ratio} on either axis, got {sw}x{sh} -> "
                         f"{tw}x{th}")


def _area_weights(dst_n: int, src_n: int) -> np.ndarray:
    """[dst_n, src_n] int64: the overlap of [d * src_n, (d + 1) * src_n) and [j * dst_n, (j + 1) * dst_n)."""
    d = np.arange(dst_n, dtype=np.int64)[:, None]
    j = np.arange(src_n, dtype=np.int64)[None, :]
    return np.maximum(np.minimum((d + 1) * src_n, (j + 1) * dst_n) - np.maximum(d * src_n, j * dst_n), 0)


def resize_area(img: np.ndarray, target_size, bits: int = 8) -> np.ndarray:
    """The area filter of the device resize (csrc/resize.hip.h) on a uint8 (bits=8) or uint16 (bits=10)
    [H,W] plane, target_size = (W, H) no larger than the plane on either axis: every destination sample is the mean of
    the source area it covers, the weights the overlap lengths in units of 1 / n_dst of a source sample, in integers:
    out = (N + D // 2) // D with D = sw * sh.  At 10 bits samples above 1023 read as 1023; equal size is the plane."""
    tw, th = int(target_size[0]), int(target_size[1])
    sh, sw = img.shape[:2]
    if bits not in (8, 10):
        raise ValueError(f"bits must be 8 or 10, got {bits!r}")
    if tw < 1 or th < 1:
        raise ValueError(f"target_size must be positive, got {target_size!r}")
    check_area(sh, sw, th, tw)
    if (sh, sw) == (th, tw):
        return img
    v = img.astype(np.int64)
    if bits == 10:
        v = np.minimum(v, 1023)
    n = _area_weights(th, sh) @ v @ _area_weights(tw, sw).T   # < 2^24 * 2^24 * 1023: int64
    d = sw * sh
    return ((n + d // 2) // d).astype(img.dtype)


def write_png(path: str, img: np.ndarray) -> None:
    """8-bit gray [H,W] or RGB [H,W,3] -> PNG (filter 0, zlib level 6)."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    if img.ndim == 2:
        ctype, rowbytes = 0, img.shape[1]
    elif img.ndim == 3 and img.shape[2] == 3:
        ctype, rowbytes = 2, img.shape[1] * 3
    else:
        raise ValueError("expected uint8 [H,W] or [H,W,3]")
    h, w = img.shape[:2]
    raw = np.zeros((h, rowbytes + 1), dtype=np.uint8)
    raw[:, 1:] = img.reshape(h, rowbytes)

    def chunk(tag, body):
        return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xffffffff)

    with open(path, "wb") as f:
        f.write(_PNG_SIG + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)) + chunk(b"IEND", b""))


# ---- uncompressed video: YUV4MPEG2 (.y4m) ------------------------------------------------------------
# The reference writes its result videos with imageio.mimsave (codec via ffmpeg,
# /root/reference/model/inference.py:176-202) and has no video READER at all (main.py's `video` command
# imports a class that does not exist).  There is no codec in this image; Y4M is the
# uncompressed container every player / ffmpeg reads and writes (`ffmpeg -i in.mp4 in.y4m`), which makes
# FrameInterpolator.interpolate_video work on real video files: header line
# "YUV4MPEG2 W<w> H<h> F<num>:<den> [I<p>] [A<n>:<d>] [C<colourspace>]", then per frame "FRAME\n" + planes.
def _y4m_header(data: bytes):
    """Parse the stream header -> (fields, offset of the first FRAME marker).  fields: width, height, fps (num, den),
    colourspace (the `C` tag, "420jpeg" when absent), colour_range ("FULL" / "LIMITED" from an `XCOLORRANGE=` token,
    None when absent), chroma (rows, cols) of each of U and V ((0, 0) for mono), frame_bytes.  8-bit streams only."""
    hdr, pos = _y4m_fields(data)
    cs = hdr["colourspace"]
    if any(c in cs for c in ("p10", "p12", "p14", "p16", "mono16")):
        raise ValueError(f"unsupported Y4M bit depth C{cs}")
    return hdr, pos


def _y4m_fields(data: bytes):
    """`_y4m_header` without the bit-depth check (frame_bytes counts one byte per sample)."""
    nl = data.index(b"\n")
    head = data[:nl].split(b" ")
    if head[0] != b"YUV4MPEG2":
        raise ValueError("not a YUV4MPEG2 stream")
    w = h = None
    fps, cs, rng = (30, 1), "420jpeg", None
    for tok in head[1:]:
        if tok[:1] == b"W":
            w = int(tok[1:])
        elif tok[:1] == b"H":
            h = int(tok[1:])
        elif tok[:1] == b"F":
            n, d = tok[1:].split(b":")
            fps = (int(n), int(d))
        elif tok[:1] == b"C":
            cs = tok[1:].decode()
        elif tok.startswith(b"XCOLORRANGE="):
            rng = tok[len(b"XCOLORRANGE="):].decode().upper()
            if rng not in ("FULL", "LIMITED"):
                raise ValueError(f"Y4M: unknown XCOLORRANGE={rng}")
    if not w or not h:
        raise ValueError("Y4M header without W/H")
    if cs.startswith("mono"):
        cw = ch = 0
    elif cs.startswith("420"):
        cw, ch = (w + 1) // 2, (h + 1) // 2
    elif cs.startswith("422"):
        cw, ch = (w + 1) // 2, h
    elif cs.startswith("444") and "alpha" not in cs:
        cw, ch = w, h
    else:
        raise ValueError(f"unsupported Y4M colourspace C{cs}")
    return dict(width=w, height=h, fps=fps, colourspace=cs, colour_range=rng, chroma=(ch, cw),
                frame_bytes=w * h + 2 * cw * ch), nl + 1


def _y4m_payloads(data: bytes, pos: int, fsz: int) -> list:
    """Offsets of the frame payloads from `pos` on (each after its FRAME line)."""
    offs = []
    while pos < len(data):
        e = data.index(b"\n", pos)
        if not data[pos:e].startswith(b"FRAME"):
            raise ValueError("Y4M: FRAME marker expected")
        pos = e + 1
        if pos + fsz > len(data):
            raise ValueError("Y4M: truncated frame")
        offs.append(pos)
        pos += fsz
    if not offs:
        raise ValueError("Y4M: no frames")
    return offs


def read_y4m(path: str):
    """-> (y [N, H, W] uint8, chroma or None, fps (num, den), colourspace tag).  `chroma` is a pair of
    [N, Hc, Wc] uint8 arrays (U, V) for the 4:2:0 / 4:2:2 / 4:4:4 layouts, None for mono."""
    with open(path, "rb") as f:
        data = f.read()
    hdr, pos = _y4m_header(data)
    w, h, (ch, cw), fsz = hdr["width"], hdr["height"], hdr["chroma"], hdr["frame_bytes"]
    ys, us, vs = [], [], []
    for off in _y4m_payloads(data, pos, fsz):
        fr = np.frombuffer(data, np.uint8, fsz, off)
        ys.append(fr[:w * h].reshape(h, w))
        if cw:
            us.append(fr[w * h:w * h + cw * ch].reshape(ch, cw))
            vs.append(fr[w * h + cw * ch:].reshape(ch, cw))
    chroma = (np.stack(us), np.stack(vs)) if cw else None
    return np.stack(ys), chroma, hdr["fps"], hdr["colourspace"]


def read_y4m_packed(path: str):
    """-> (frames [N, frame_bytes] uint8, header fields as `_y4m_header` returns them).  Each row is one frame payload
    as stored (Y, then U, then V): for 4:2:0 the packed I420 frame that `FrameInterpolationUNet.forward_yuv420` takes."""
    with open(path, "rb") as f:
        data = f.read()
    hdr, pos = _y4m_header(data)
    fsz = hdr["frame_bytes"]
    frames = np.stack([np.frombuffer(data, np.uint8, fsz, off) for off in _y4m_payloads(data, pos, fsz)])
    return frames, hdr


def write_y4m(path: str, y: np.ndarray, chroma=None, fps=(30, 1), colourspace: str = None,
              colour_range: str = None) -> None:
    """y: [N, H, W] uint8; chroma: None (-> Cmono) or (U, V) planes as read_y4m returns them.  colour_range: None (no
    XCOLORRANGE token: the header is byte for byte what it always was), "FULL" or "LIMITED"."""
    y = np.ascontiguousarray(y, dtype=np.uint8)
    n, h, w = y.shape
    cs = colourspace or ("mono" if chroma is None else "420jpeg")
    if (chroma is None) != cs.startswith("mono"):
        raise ValueError("chroma planes and colourspace tag disagree")
    head = _y4m_header_line(w, h, fps, cs, colour_range, 8)
    with open(path, "wb") as f:
        f.write(head)
        for i in range(n):
            f.write(b"FRAME\n")
            f.write(y[i].tobytes())
            if chroma is not None:
                f.write(np.ascontiguousarray(chroma[0][i], dtype=np.uint8).tobytes())
                f.write(np.ascontiguousarray(chroma[1][i], dtype=np.uint8).tobytes())


# ---- 10-bit Y4M: every sample a 10-bit code in a little-endian 16-bit word -----------------------------------------
# The tags ffmpeg writes for yuv420p10le / yuv422p10le / yuv444p10le / gray10le (`ffmpeg -i in.mkv in.y4m` keeps a
# 10-bit source's format): "C420p10 XYSCSS=420P10" and so on, "Cmono10".  12-, 14- and 16-bit streams are refused
# (the colour conversion of DESIGN.md 3.3d is defined for 10 bits).
Y4M_P10_TAGS = ("420p10", "422p10", "444p10", "mono10")


def _y4m_header_p10(data: bytes):
    hdr, pos = _y4m_fields(data)
    cs = hdr["colourspace"]
    if cs not in Y4M_P10_TAGS:
        if any(c in cs for c in ("p9", "p12", "p14", "p16", "mono9", "mono12", "mono14", "mono16")):
            raise ValueError(f"unsupported Y4M bit depth C{cs}: the 10-bit reader takes "
                             f"{', '.join('C' + t for t in Y4M_P10_TAGS)}")
        raise ValueError(f"Y4M colourspace C{cs} is not a 10-bit layout ({', '.join('C' + t for t in Y4M_P10_TAGS)}): "
                         "read 8-bit video with read_y4m")
    samples = hdr["frame_bytes"]
    hdr.update(bits=10, frame_samples=samples, frame_bytes=2 * samples)
    return hdr, pos


def read_y4m_packed_p10(path: str):
    """-> (frames [N, frame_samples] uint16, header fields as `_y4m_header` returns them plus bits = 10 and
    frame_samples; frame_bytes counts the 2 bytes per sample).  Each row is one frame payload (Y, then U, then V):
    for C420p10 the packed frame that `FrameInterpolationUNet.forward_yuv420p10` takes.  Samples are read as stored
    (values above 1023 included; the device kernels read those as 1023)."""
    with open(path, "rb") as f:
        data = f.read()
    hdr, pos = _y4m_header_p10(data)
    n = hdr["frame_samples"]
    frames = np.stack([np.frombuffer(data, "<u2", n, off) for off in _y4m_payloads(data, pos, hdr["frame_bytes"])])
    return frames.astype(np.uint16), hdr


def read_y4m_p10(path: str):
    """`read_y4m` for 10-bit streams -> (y [N, H, W] uint16, chroma or None, fps (num, den), colourspace tag)."""
    frames, hdr = read_y4m_packed_p10(path)
    w, h, (ch, cw) = hdr["width"], hdr["height"], hdr["chroma"]
    n, ny, nc = frames.shape[0], w * h, cw * ch
    y = frames[:, :ny].reshape(n, h, w)
    chroma = None
    if cw:
        chroma = (frames[:, ny:ny + nc].reshape(n, ch, cw), frames[:, ny + nc:].reshape(n, ch, cw))
    return y, chroma, hdr["fps"], hdr["colourspace"]


def write_y4m_p10(path: str, y: np.ndarray, chroma=None, fps=(30, 1), colourspace: str = None,
                  colour_range: str = None) -> None:
    """y: [N, H, W] uint16 10-bit codes; chroma: None (-> Cmono10) or (U, V) planes as read_y4m_p10 returns them
    (-> C420p10 unless `colourspace` says 422p10 / 444p10).  Samples go out as little-endian 16-bit words, with the
    header ffmpeg writes (`C420p10 XYSCSS=420P10`); colour_range: None (no XCOLORRANGE token), "FULL" or "LIMITED"."""
    y = np.ascontiguousarray(y, dtype=np.uint16)
    n, h, w = y.shape
    cs = colourspace or ("mono10" if chroma is None else "420p10")
    if cs not in Y4M_P10_TAGS:
        raise ValueError(f"colourspace must be one of {Y4M_P10_TAGS}, got {cs!r}")
    if (chroma is None) != cs.startswith("mono"):
        raise ValueError("chroma planes and colourspace tag disagree")
    head = _y4m_header_line(w, h, fps, cs, colour_range, 10)
    with open(path, "wb") as f:
        f.write(head)
        for i in range(n):
            f.write(b"FRAME\n")
            f.write(y[i].astype("<u2").tobytes())
            if chroma is not None:
                f.write(np.ascontiguousarray(chroma[0][i], dtype=np.uint16).astype("<u2").tobytes())
                f.write(np.ascontiguousarray(chroma[1][i], dtype=np.uint16).astype("<u2").tobytes())


def y4m_colourspace(path: str) -> str:
    """The `C` tag of a Y4M file's stream header ("420jpeg" when absent), read from its first line only."""
    with open(path, "rb") as f:
        line = f.readline(4096)
    for tok in line.rstrip(b"\n").split(b" ")[1:]:
        if tok[:1] == b"C":
            return tok[1:].decode()
    return "420jpeg"


def y4m_interlace(header_line: bytes):
    """The `I` token of a Y4M stream header line: "p" (progressive), "t" (interlaced, top field first), "b" (bottom
    field first), "m" (mixed), or None where the header has none; any other text as it stands (the readers never
    refused one).  (The header dicts of the readers do not carry it: `Y4MReader.interlace` does.)"""
    for tok in header_line.rstrip(b"\n").split(b" ")[1:]:
        if tok[:1] == b"I":
            return tok[1:].decode(errors="replace")
    return None


def _y4m_header_line(w: int, h: int, fps, cs: str, colour_range, bits: int) -> bytes:
    """The stream header `write_y4m` (bits 8) / `write_y4m_p10` (bits 10) write: 10-bit layouts other than mono carry
    ffmpeg's `XYSCSS=` token; `XCOLORRANGE=` only when colour_range is given."""
    ext = "" if bits == 8 or cs.startswith("mono") else f" XYSCSS={cs.upper()}"
    if colour_range is not None:
        if colour_range.upper() not in ("FULL", "LIMITED"):
            raise ValueError(f"colour_range must be FULL or LIMITED, got {colour_range!r}")
        ext += f" XCOLORRANGE={colour_range.upper()}"
    return f"YUV4MPEG2 W{w} H{h} F{int(fps[0])}:{int(fps[1])} Ip A1:1 C{cs}{ext}\n".encode()


# ---- incremental Y4M: a stream of any length through a bounded buffer (stream.py) -------------------
def _y4m_stream_header(line: bytes, bits):
    """Header fields of one header line (with its newline) as `_y4m_header` (8-bit) or `_y4m_header_p10` (10-bit)
    return them, plus `bits`.  bits None picks the reader from the tag; 8 or 10 applies that reader's checks."""
    if bits is None:
        tag = b"420jpeg"
        for tok in line.rstrip(b"\n").split(b" ")[1:]:
            if tok[:1] == b"C":
                tag = tok[1:]
        bits = 10 if tag.decode(errors="replace") in Y4M_P10_TAGS else 8
    if bits == 10:
        hdr, _ = _y4m_header_p10(line)
    elif bits == 8:
        hdr, _ = _y4m_header(line)
        hdr.update(bits=8, frame_samples=hdr["frame_bytes"])
    else:
        raise ValueError(f"bits must be None, 8 or 10, got {bits!r}")
    return hdr


class Y4MReader:
    """Frame-at-a-time YUV4MPEG2 reader.  `src`: a path or a readable binary file object (a pipe, `sys.stdin.buffer`);
    it is never seeked and nothing past the frames asked for is read from it.  The header is read on construction; its
    fields (`width`, `height`, `fps`, `colourspace`, `colour_range`, `chroma`, `frame_bytes`, `frame_samples`, `bits`)
    are those of `_y4m_header` / `_y4m_header_p10`, also as attributes.  bits: None (8 or 10 from the tag), or 8 / 10
    to apply that whole-file reader's bit-depth checks and messages.

    `read_into(buf, max_frames)` fills rows 0.. of a caller-owned C-contiguous array (any dtype; each row holds
    `frame_bytes` bytes: uint8 [M, frame_bytes], uint16 [M, frame_samples], or the numpy view of a pinned tensor) with
    the next frame payloads and returns how many it read: fewer than asked only at the end of the stream."""

    def __init__(self, src, bits=None):
        self._own = isinstance(src, (str, bytes, os.PathLike))
        self._f = open(src, "rb") if self._own else src
        try:
            line = self._f.readline()
            if not line.startswith(b"YUV4MPEG2"):
                raise ValueError("not a YUV4MPEG2 stream")
            if not line.endswith(b"\n"):
                raise ValueError("Y4M: truncated stream header")
            self.header = _y4m_stream_header(line, bits)
            self.interlace = y4m_interlace(line)   # (not a key of `header`)
        except BaseException:
            self.close()
            raise
        for k, v in self.header.items():
            setattr(self, k, v)
        self.frames_read = 0
        self._eof = False

    def _fill(self, mv: memoryview) -> int:
        got = 0
        readinto = getattr(self._f, "readinto", None)
        while got < len(mv):
            if readinto is not None:
                k = readinto(mv[got:])
            else:
                b = self._f.read(len(mv) - got)
                k = len(b)
                mv[got:got + k] = b
            if not k:
                break
            got += k
        return got

    def read_into(self, buf: np.ndarray, max_frames: int = None) -> int:
        rows = buf.reshape(buf.shape[0], -1) if buf.ndim != 2 else buf
        if not rows.flags.c_contiguous or rows[0].nbytes != self.frame_bytes:
            raise ValueError(f"read_into needs a C-contiguous array of rows of {self.frame_bytes} bytes, "
                             f"got {buf.dtype} {buf.shape}")
        want = rows.shape[0] if max_frames is None else min(int(max_frames), rows.shape[0])
        n = 0
        while n < want and not self._eof:
            line = self._f.readline()
            if not line:
                self._eof = True
                break
            if not line.startswith(b"FRAME") or not line.endswith(b"\n"):
                raise ValueError("Y4M: FRAME marker expected")
            mv = memoryview(rows[n]).cast("B")
            if self._fill(mv) < len(mv):
                raise ValueError("Y4M: truncated frame")
            n += 1
        self.frames_read += n
        if self._eof and not self.frames_read:
            raise ValueError("Y4M: no frames")
        return n

    def close(self) -> None:
        if self._own:
            self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def y4m_frame_count(path) -> int:
    """Frames in a Y4M file, by a pass that reads the FRAME lines and seeks past the payloads (a regular file only:
    the frame count of a pipe is not known before it has been read)."""
    with Y4MReader(path) as r:
        f = r._f
        size = os.fstat(f.fileno()).st_size
        n = 0
        while True:
            line = f.readline()
            if not line:
                break
            if not line.startswith(b"FRAME") or not line.endswith(b"\n"):
                raise ValueError("Y4M: FRAME marker expected")
            if f.tell() + r.frame_bytes > size:
                raise ValueError("Y4M: truncated frame")
            f.seek(r.frame_bytes, os.SEEK_CUR)
            n += 1
        if not n:
            raise ValueError("Y4M: no frames")
        return n


class Y4MWriter:
    """Frame-at-a-time YUV4MPEG2 writer.  `dst`: a path or a writable binary file object.  The header is written on
    construction, byte for byte what `write_y4m` (bits 8; colourspace default "420jpeg") / `write_y4m_p10` (bits 10;
    default "420p10") write for the same arguments.  `write(frames)` appends each row of a C-contiguous array (rows of
    `frame_bytes` bytes: packed Y, U, V payloads; 16-bit samples in the host's little-endian order) behind a
    `FRAME` line, straight from the array's memory (a pinned slot included): no per-frame copy."""

    def __init__(self, dst, width: int, height: int, fps=(30, 1), colourspace: str = None, colour_range: str = None,
                 bits: int = 8):
        if bits == 10:
            cs = colourspace or "420p10"
            if cs not in Y4M_P10_TAGS:
                raise ValueError(f"colourspace must be one of {Y4M_P10_TAGS}, got {cs!r}")
        elif bits == 8:
            cs = colourspace or "420jpeg"
        else:
            raise ValueError(f"bits must be 8 or 10, got {bits!r}")
        head = _y4m_header_line(int(width), int(height), fps, cs, colour_range, bits)
        self.header = _y4m_stream_header(head, bits)
        self.frame_bytes = self.header["frame_bytes"]
        self.frames_written = 0
        self._own = isinstance(dst, (str, bytes, os.PathLike))
        self._f = open(dst, "wb") if self._own else dst
        self._f.write(head)

    def write(self, frames: np.ndarray) -> None:
        if frames.shape[0] == 0:
            return
        rows = frames.reshape(frames.shape[0], -1)
        if not rows.flags.c_contiguous or rows[0].nbytes != self.frame_bytes:
            raise ValueError(f"write needs C-contiguous rows of {self.frame_bytes} bytes, got {frames.dtype} "
                             f"{frames.shape}")
        if rows.dtype.itemsize > 1 and rows.dtype.byteorder == ">":
            raise ValueError("16-bit samples must be little-endian")
        for row in rows:
            self._f.write(b"FRAME\n")
            self._f.write(memoryview(row).cast("B"))
        self.frames_written += rows.shape[0]

    def flush(self) -> None:
        self._f.flush()

    def close(self) -> None:
        if self._own:
            self._f.close()
        else:
            self._f.flush()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
