"""CPU replay of ``pool_recipe_kernel``'s per-slot draws (``csrc/pool_recipe.hip``) from the Philox
mirror of ``sampler_oracles``: numpy only, fp64 arithmetic on the kernel's exact fp32 uniforms.

Slot ``s`` of a pool of ``P`` slots in batches of ``B`` at pool counter ``pc`` draws from the
counter ``(gb, t) = (pc * P/B + s // B, s % B)``, key ``(seed, 0xA5A5A5A5)``, stream words
0x5eed (flip: ``.z & 1``), 0x5ef0..0x5ef4 (box attempts), 0x5ef5 (top, left), 0x5ef8 (factors)
and 0x5ef9 (order code), as the README documents them."""
import math

import numpy as np

import sampler_oracles as so

K1 = 0xA5A5A5A5
W_CROP, W_BOX, W_POS, W_FACTORS, W_ORDER = 0x5eed, 0x5ef0, 0x5ef5, 0x5ef8, 0x5ef9


def slot_words(seed, pc, P, B, word):
    """The four 32-bit words of every slot's Philox call with stream word ``word``: [4][P]."""
    s = np.arange(P, dtype=np.uint64)
    gb = np.uint64(pc * (P // B)) + s // np.uint64(B)
    r = so.philox4x32((gb & so.U32, gb >> np.uint64(32), s % np.uint64(B), word), seed, K1)
    return np.stack([np.asarray(x, dtype=np.uint64) for x in r])


def u01(x):
    return (int(x) >> 8) * 2.0 ** -24


def flips(seed, pc, P, B):
    return (slot_words(seed, pc, P, B, W_CROP)[2] & np.uint64(1)).astype(np.int64)


def fallback_box(Hs, Ws, rrc):
    _, _, rlo, rhi = rrc
    h, w = Hs, Ws
    if Ws / Hs < rlo:
        h = int(round(Ws / rlo))
    elif Ws / Hs > rhi:
        w = int(round(Hs * rhi))
    return (Hs - h) // 2, (Ws - w) // 2, h, w


def boxes(seed, pc, P, B, Hs, Ws, rrc):
    """Per slot ``(attempt, top, left, h, w, risky)`` in fp64.  ``risky``: some attempt up to the
    accepted one had ``sqrt(...)`` within 1e-3 of a half-integer, where fp32 may round the other
    way."""
    slo, shi, rlo, rhi = rrc
    att = [slot_words(seed, pc, P, B, W_BOX + k) for k in range(5)]
    pos = slot_words(seed, pc, P, B, W_POS)
    out = []
    for s in range(P):
        risky, got = False, None
        for k in range(10):
            r = att[k // 2][:, s]
            us, ur = (r[2], r[3]) if k & 1 else (r[0], r[1])
            target = Hs * Ws * (slo + (shi - slo) * u01(us))
            aspect = math.exp(math.log(rlo) + (math.log(rhi) - math.log(rlo)) * u01(ur))
            wf, hf = math.sqrt(target * aspect), math.sqrt(target / aspect)
            risky |= any(abs(v - math.floor(v) - 0.5) < 1e-3 for v in (wf, hf))
            w, h = int(round(wf)), int(round(hf))
            if 0 < w <= Ws and 0 < h <= Hs:
                got = (k, int(pos[0, s]) % (Hs - h + 1), int(pos[1, s]) % (Ws - w + 1), h, w)
                break
        if got is None:
            got = (10,) + fallback_box(Hs, Ws, rrc)
        out.append(got + (risky,))
    return out


def jitter_draws(seed, pc, P, B, jitter):
    """Per slot ``(fb, fc, fs, fh, code)`` in fp64."""
    f = slot_words(seed, pc, P, B, W_FACTORS)
    o = slot_words(seed, pc, P, B, W_ORDER)
    out = []
    for s in range(P):
        v = []
        for k in range(3):
            lo, hi = max(0.0, 1.0 - jitter[k]), 1.0 + jitter[k]
            v.append(lo + (hi - lo) * u01(f[k, s]))
        v.append(-jitter[3] + 2.0 * jitter[3] * u01(f[3, s]))
        out.append(tuple(v) + (int(o[0, s]) % 24,))
    return out


def order_of(code):
    """The Lehmer decoding the README documents (0 brightness, 1 contrast, 2 saturation, 3 hue)."""
    rest = [0, 1, 2, 3]
    return [rest.pop(code // 6), rest.pop(code % 6 // 2), rest.pop(code % 2), rest[0]]


def box_coverage(bx, H, W, Hs, Ws):
    """(some box smaller than the output, some larger, some touching an image edge)."""
    small = any(h < H and w < W for _, _, _, h, w, _ in bx)
    large = any(h > H and w > W for _, _, _, h, w, _ in bx)
    edge = any(t == 0 or l == 0 or t + h == Hs or l + w == Ws for _, t, l, h, w, _ in bx)
    return small, large, edge


def contrast_coverage(draws):
    """(positions 0..3 at which contrast stands, operations that precede it somewhere)."""
    pos, before = set(), set()
    for d in draws:
        order = order_of(d[4])
        k = order.index(1)
        pos.add(k)
        before.update(order[:k])
    return pos, before
