"""numpy restatement of the 10-bit 4:2:2 wire packings, written from the table there, sample by sample:
where sample (y, x) of a plane lies in a wire frame, as an index formula - no group loops, no shared code with the package.

Working format (yuv422p10le): one frame is uint16 words holding the code, Y H x W at y * W + x, then U at H*W + y * Wc + j,
then V at H*W + H*Wc + y * Wc + j, Wc = ceil(W / 2).

  v210    32-bit little-endian words, three 10-bit fields each (field f at bits 10 f); 16 bytes per 6 pixels; a row is
          128 * ceil(W / 48) bytes.  Pixel x = 6 g + r: Y is field _V210_Y[r] of the group, chroma j = 3 g + k: U is field
          _V210_U[k], V is field _V210_V[k] (a field number counts 0..11 through the group's four words).
  y210le  16-bit words, code << 6: Y(x) at word 2 x, U(j) at word 4 j + 1, V(j) at word 4 j + 3; a row is 2 W words.
  p210le  16-bit words, code << 6: Y(y, x) at y * W + x; U(y, j) at H*W + y * 2 Wc + 2 j, V one word later.
"""
import numpy as np

PACKINGS = ("v210", "y210le", "p210le")
CODES = {"v210": 0, "y210le": 1, "p210le": 2}

# field numbers inside a group: word = n // 3, shift = 10 * (n % 3)
_V210_Y = (1, 3, 5, 7, 9, 11)     # w0 mid, w1 low, w1 high, w2 mid, w3 low, w3 high
_V210_U = (0, 4, 8)               # w0 low, w1 mid, w2 high
_V210_V = (2, 6, 10)              # w0 high, w2 low, w3 mid


def row_bytes(packing, w):
    """Bytes of one tight row of a one-plane packing."""
    return {"v210": 128 * -(-w // 48), "y210le": 4 * w}[packing]


def frame_bytes(packing, h, w):
    if packing == "p210le":
        return 2 * (h * w + 2 * h * -(-w // 2))
    if w % 2:
        raise ValueError("odd width")
    return h * row_bytes(packing, w)


def planar_samples(h, w):
    return h * w + 2 * h * -(-w // 2)


def planes(planar, h, w):
    """[..., samples] uint16 -> Y [..., h, w], U, V [..., h, wc] (views)."""
    wc = -(-w // 2)
    lead = planar.shape[:-1]
    y = planar[..., :h * w].reshape(lead + (h, w))
    u = planar[..., h * w:h * w + h * wc].reshape(lead + (h, wc))
    v = planar[..., h * w + h * wc:h * w + 2 * h * wc].reshape(lead + (h, wc))
    return y, u, v


def _v210_place(field_of, idx, per_group):
    """Plane columns `idx` -> (32-bit word index in the row, shift)."""
    g, r = np.divmod(idx, per_group)
    n = np.asarray(field_of)[r]
    return 4 * g + n // 3, 10 * (n % 3)


def pack(planar, h, w, packing, pitch=None):
    """uint16 [B, samples] (any word; above 1023 packs as 1023) -> the tight wire frames as uint8 [B, frame_bytes]; with
    `pitch` (bytes, one-plane packings) rows that far apart instead, the bytes behind the tight row zero."""
    planar = np.minimum(np.asarray(planar, dtype=np.uint16), 1023)
    b = planar.shape[0]
    y, u, v = planes(planar, h, w)
    wc = -(-w // 2)
    xs, js = np.arange(w), np.arange(wc)
    if packing == "p210le":
        out = np.zeros((b, h * w + 2 * h * wc), dtype=np.uint16)
        out[:, :h * w] = (y << 6).reshape(b, -1)
        c = out[:, h * w:].reshape(b, h, 2 * wc)
        c[:, :, 2 * js] = u << 6
        c[:, :, 2 * js + 1] = v << 6
        return out.view(np.uint8)
    if w % 2:
        raise ValueError("odd width")
    row = row_bytes(packing, w)
    pitch = row if pitch is None else pitch
    if packing == "y210le":
        out = np.zeros((b, h, pitch // 2), dtype=np.uint16)
        out[:, :, 2 * xs] = y << 6
        out[:, :, 4 * js + 1] = u << 6
        out[:, :, 4 * js + 3] = v << 6
        return out.reshape(b, -1).view(np.uint8)
    out = np.zeros((b, h, pitch // 4), dtype=np.uint32)
    for plane, field_of, idx, per in ((y, _V210_Y, xs, 6), (u, _V210_U, js, 3), (v, _V210_V, js, 3)):
        word, shift = _v210_place(field_of, idx, per)
        np.bitwise_or.at(out, (slice(None), slice(None), word), plane.astype(np.uint32) << shift.astype(np.uint32))
    return out.reshape(b, -1).view(np.uint8)


def unpack(wire, h, w, packing, pitch=None):
    """uint8 [B, frame bytes] wire frames (tight, or one-plane rows `pitch` bytes apart) -> uint16 [B, samples]."""
    wire = np.ascontiguousarray(wire)
    b = wire.shape[0]
    wc = -(-w // 2)
    xs, js = np.arange(w), np.arange(wc)
    out = np.empty((b, planar_samples(h, w)), dtype=np.uint16)
    y, u, v = planes(out, h, w)
    if packing == "p210le":
        words = wire.view(np.uint16)
        y[...] = words[:, :h * w].reshape(b, h, w) >> 6
        c = words[:, h * w:h * w + 2 * h * wc].reshape(b, h, 2 * wc)
        u[...] = c[:, :, 2 * js] >> 6
        v[...] = c[:, :, 2 * js + 1] >> 6
        return out
    pitch = row_bytes(packing, w) if pitch is None else pitch
    if packing == "y210le":
        words = wire.view(np.uint16).reshape(b, h, pitch // 2)
        y[...] = words[:, :, 2 * xs] >> 6
        u[...] = words[:, :, 4 * js + 1] >> 6
        v[...] = words[:, :, 4 * js + 3] >> 6
        return out
    words = wire.view(np.uint32).reshape(b, h, pitch // 4)
    for plane, field_of, idx, per in ((y, _V210_Y, xs, 6), (u, _V210_U, js, 3), (v, _V210_V, js, 3)):
        word, shift = _v210_place(field_of, idx, per)
        plane[...] = (words[:, :, word] >> shift.astype(np.uint32)) & 1023
    return out
