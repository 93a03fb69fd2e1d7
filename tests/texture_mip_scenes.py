"""Mip chains, scenes and the numpy restatement of mip-mapped texture sampling (csrc/texture.hpp, csrc/texture_host.hpp) for
test_texture_mips_*.py.  tests/texture_scenes.py holds the single-level sampler this builds on.

The chain and the sampler are restated one numpy float32 operation per device operation and compared bit for bit.  The level
selection is restated twice: in float32, operation for operation (`footprint_lod32`), and in float64 from the ray, the mesh
and the uvs alone (`lod_of_rays`), which is what the geometry tests compare the device with."""
import os

import numpy as np

import texture_scenes as TS

F32 = np.float32
NEAREST, MIPMAP, MIPS_GIVEN = 0x1, 0x10, 0x20
CHAIN_SIZES = ((1, 1), (1, 7), (5, 3), (8, 8), (16, 4), (33, 17))    # (width, height)
GEOMETRY_SIZES = CHAIN_SIZES + ((65536, 1),)
BOUNCE_SPREAD = 0.125            # kTexBounceSpread
BAR = 2.0 ** -10                 # of a level: moves a colour in [0, 1] by less than half a UNORM8 step


# ------------------------------------------------------------------------------------------------ the chain
def chain_dims(w, h):
    """[(width, height)] of every level: max(1, W >> l) x max(1, H >> l), floor(log2(max(W, H))) + 1 levels"""
    levels = int(max(w, h)).bit_length()
    return [(max(1, w >> l), max(1, h >> l)) for l in range(levels)]


def downsample(im):
    """level l + 1 from level l ([H, W, 4] float32): ((a + b) + (c + d)) * 0.25f, columns and rows clamped to the level"""
    im = np.asarray(im, F32)
    h, w = im.shape[:2]
    dw, dh = max(1, w >> 1), max(1, h >> 1)
    x0, x1 = np.minimum(2 * np.arange(dw), w - 1), np.minimum(2 * np.arange(dw) + 1, w - 1)
    y0, y1 = np.minimum(2 * np.arange(dh), h - 1), np.minimum(2 * np.arange(dh) + 1, h - 1)
    a, b = im[y0][:, x0], im[y0][:, x1]
    c, d = im[y1][:, x0], im[y1][:, x1]
    return (((a + b).astype(F32) + (c + d).astype(F32)).astype(F32) * F32(0.25)).astype(F32)


def build_chain(im):
    """every level of the generated chain of level 0 `im`"""
    out = [np.asarray(im, F32)]
    while out[-1].shape[0] > 1 or out[-1].shape[1] > 1:
        out.append(downsample(out[-1]))
    assert [(l.shape[1], l.shape[0]) for l in out] == chain_dims(im.shape[1], im.shape[0])
    return out


def random_image(w, h, seed):
    return np.random.default_rng(seed).uniform(0.0, 1.0, (h, w, 4)).astype(F32)


def random_chain(w, h, seed):
    """a chain no box filter made: every level random, so a sampler that reads a given chain must read THESE texels"""
    return [random_image(lw, lh, seed * 100 + l) for l, (lw, lh) in enumerate(chain_dims(w, h))]


def chain_atlas(chains, flags, given, pad=3):
    """(textures [n, 4] u32, texels [m, 4] f32) of the chains (lists of levels): `given` puts every level of a chain behind its
    level 0 and sets RTPT_TEX_MIPS_GIVEN; otherwise the atlas holds the levels 0 alone.  `pad` sentinel texels (-1000) in front
    of every texture, as texture_scenes.atlas does"""
    desc, parts, first = [], [], 0
    for ch in chains:
        parts.append(np.full((pad, 4), -1000.0, F32))
        first += pad
        h, w = ch[0].shape[:2]
        desc.append((w, h, first, flags | MIPMAP | (MIPS_GIVEN if given else 0)))
        for level in (ch if given else ch[:1]):
            parts.append(np.asarray(level, F32).reshape(-1, 4))
            first += level.shape[0] * level.shape[1]
    return np.array(desc, np.uint32).reshape(-1, 4), np.concatenate(parts)


# ------------------------------------------------------------------------------------------------ the sampler at a level
def clamp_lod(lam, levels):
    """lambda > 0 ? lambda : 0 (a NaN too), then lambda < L - 1 ? lambda : L - 1"""
    lam = np.asarray(lam, F32)
    with np.errstate(invalid="ignore"):
        lam = np.where(lam > 0, lam, F32(0)).astype(F32)
        return np.where(lam < F32(levels - 1), lam, F32(levels - 1)).astype(F32)


def sample_lod(chain, flags, uv, lam):
    """[n, 4] float32: the chain (list of [h, w, 4] levels) at uv [n, 2] and level lam [n] (any bit pattern)"""
    uv = np.asarray(uv, F32).reshape(-1, 2)
    L = len(chain)
    lam = clamp_lod(np.broadcast_to(np.asarray(lam, F32), (len(uv),)), L)

    def level(l):     # every uv at its own level l [n]
        out = np.zeros((len(uv), 4), F32)
        for k in np.unique(l):
            m = l == k
            im = chain[int(k)]
            out[m] = TS.sample(im.reshape(-1, 4), (im.shape[1], im.shape[0], 0, flags & NEAREST), uv[m])
        return out
    if flags & NEAREST:
        return level(np.clip(np.floor((lam + F32(0.5)).astype(F32)).astype(np.int64), 0, L - 1))
    l0 = np.clip(np.floor(lam).astype(np.int64), 0, L - 1)
    f = (lam - l0.astype(F32)).astype(F32)
    a = level(l0)
    b = level(np.minimum(l0 + 1, L - 1))
    return np.where((f > 0)[:, None], TS._lerp(a, b, f), a).astype(F32)


# ------------------------------------------------------------------------------------------------ the level selection
def plog2(x):
    """piecewise-linear log2 of positive finite float32: (float)(exponent) + (float)(mantissa bits) * 2^-23"""
    b = np.asarray(x, F32).view(np.uint32).astype(np.int64)
    return (((b >> 23) - 127).astype(F32) + ((b & 0x7FFFFF).astype(F32) * F32(2.0 ** -23)).astype(F32)).astype(F32)


def plog2_f64(x):
    """the same function of a float64 argument: e + (m - 1) for x = m 2^e, m in [1, 2)"""
    m, e = np.frexp(np.asarray(x, np.float64))      # x = m 2^e, m in [0.5, 1)
    return (e - 1) + (2.0 * m - 1.0)


def footprint_lod32(w, nd, p, uv6, W, H):
    """texture.hpp's footprint_lod in float32, operation for operation (before the clamp).  w, nd [n]; p [n, 3, 3] the posed
    vertices; uv6 [n, 6]"""
    w, nd, p, uv6 = (np.asarray(v, F32) for v in (w, nd, p, uv6))
    e1, e2 = (p[:, 1] - p[:, 0]).astype(F32), (p[:, 2] - p[:, 0]).astype(F32)

    def cr(a, b, c, d):
        return ((a * b).astype(F32) - (c * d).astype(F32)).astype(F32)
    cx, cy, cz = cr(e1[:, 1], e2[:, 2], e1[:, 2], e2[:, 1]), cr(e1[:, 2], e2[:, 0], e1[:, 0], e2[:, 2]), cr(e1[:, 0], e2[:, 1], e1[:, 1], e2[:, 0])
    aw = np.sqrt((((cx * cx).astype(F32) + (cy * cy).astype(F32)).astype(F32) + (cz * cz).astype(F32)).astype(F32)).astype(F32)
    u0, v0, u1, v1, u2, v2 = uv6.T
    at = np.abs((cr((u1 - u0).astype(F32), (v2 - v0).astype(F32), (u2 - u0).astype(F32), (v1 - v0).astype(F32)) * (F32(W) * F32(H))).astype(F32))
    with np.errstate(all="ignore"):
        D = (at / aw).astype(F32)
        rho2 = ((((w * w).astype(F32) * D).astype(F32)) / (nd * nd).astype(F32)).astype(F32)
        ok = (D > 0) & np.isfinite(D) & (rho2 > 0) & np.isfinite(rho2)
        return np.where(ok, F32(0.5) * plog2(np.where(ok, rho2, F32(1))), F32(0)).astype(F32)


def primary_spread(slope, frame_h):
    """pix = (2.0f * slope) / (float)H"""
    return float((F32(2.0) * F32(slope)) / F32(frame_h))


def lod_of_rays(rays, tris, tri_uv, tri_texture, dims, levels, spread):
    """float64, from the ray, the mesh and the uvs alone: (id + 1 of the closest hit or 0, lambda clamped to the chain) of
    rays [n, 6] (unit directions) against the posed triangles `tris` [t, 3, 3]; triangle i reads uv record i % len(tri_uv).
    dims[k] = (W, H) and levels[k] of texture k; spread: the footprint width per unit of distance."""
    rays, tris = np.asarray(rays, np.float64).reshape(-1, 6), np.asarray(tris, np.float64)
    o, d = rays[:, None, :3], rays[:, None, 3:]
    e1, e2 = (tris[:, 1] - tris[:, 0])[None], (tris[:, 2] - tris[:, 0])[None]
    pv = np.cross(d, e2)
    det = (e1 * pv).sum(-1)
    with np.errstate(all="ignore"):
        tv = o - tris[None, :, 0]
        u = (tv * pv).sum(-1) / det
        qv = np.cross(tv, e1)
        v = (d * qv).sum(-1) / det
        t = (e2 * qv).sum(-1) / det
    hit = (np.abs(det) > 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
    t = np.where(hit, t, np.inf)
    best = t.argmin(1)
    tb = t[np.arange(len(rays)), best]
    ids = np.where(np.isfinite(tb), best + 1, 0)
    lam = np.zeros(len(rays))
    for i in np.flatnonzero(ids):
        k = best[i]
        rec = k % len(tri_uv)
        if tri_texture[rec] == 0:
            continue
        W, H = dims[tri_texture[rec] - 1]
        L = levels[tri_texture[rec] - 1]
        if L == 1:
            continue
        p = tris[k]
        n = np.cross(p[1] - p[0], p[2] - p[0])
        aw = np.linalg.norm(n)
        u0, v0, u1, v1, u2, v2 = np.asarray(tri_uv[rec], np.float64)
        at = abs((u1 - u0) * (v2 - v0) - (u2 - u0) * (v1 - v0)) * W * H
        nd = (n / aw) @ rays[i, 3:]
        rho2 = (tb[i] * spread) ** 2 * (at / aw) / nd ** 2
        lam[i] = min(max(0.5 * plog2_f64(rho2), 0.0), L - 1.0)
    return ids, lam


# ------------------------------------------------------------------------------------------------ scenes
FLOOR_CAM = (0.0, 1.0, 6.0)


def floor_mesh():
    """a floor receding from FLOOR_CAM to the horizon, y = -1, under the sky: the footprint grows from row to row, so one
    frame spans several levels.  Triangles (0, 1, 2), (2, 3, 0), not a fan pair, like texture_scenes.quad_mesh"""
    xyz = np.array([[-30, -1, 5], [30, -1, 5], [30, -1, -60], [-30, -1, -60]], F32)
    idx = np.array([[0, 1, 2], [2, 3, 0]], np.uint32)
    return xyz, idx


def floor_tri_uv(per_unit):
    """uv = (x, z) * per_unit, with a shear: u += 0.3 z per_unit"""
    xyz, idx = floor_mesh()
    u = (xyz[:, 0].astype(np.float64) + 0.3 * xyz[:, 2]) * per_unit
    v = xyz[:, 2].astype(np.float64) * per_unit
    return np.stack([u, v], -1)[idx].reshape(-1, 6).astype(F32)


def pixel_centre_rays(size, slope, cam):
    """K2's jitter-free primary ray through every pixel centre (raytrace.comp.glsl:314-320): [H * W, 6] float32"""
    W, H = size
    cx, cy = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    ux, uy = (2 * cx - W) / H, -(2 * cy - H) / H
    d = np.stack([slope * ux, slope * uy, -np.ones_like(ux)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.broadcast_to(np.asarray(cam, np.float64), d.shape)
    return np.concatenate([o, d], -1).reshape(-1, 6).astype(F32)


def rays_into(tris, n, seed, margin=0.05):
    """n unit rays [n, 6] float32 from random origins in front of (+z of) random interior points of the triangles [t, 3, 3]:
    at least `margin` in every barycentric coordinate, so no ray runs near an edge"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, len(tris), n)
    b = rng.uniform(margin, 1.0, (n, 3))
    b = margin + (1 - 3 * margin) * b / b.sum(1, keepdims=True)
    target = (np.asarray(tris, np.float64)[k] * b[:, :, None]).sum(1)
    o = target + np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.5, 1.5, n), rng.uniform(1.0, 5.0, n)], -1)
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d], -1).astype(F32)


def posed(xyz, idx, xforms=None, model=None):
    """float64 [t, 3, 3]: the mesh under the 3 x 4 instance transforms (instance i's triangles behind instance i - 1's) and the
    column-major 4 x 4 model matrix"""
    v = np.asarray(xyz, np.float64)[np.asarray(idx)]
    if xforms is not None:
        x = np.asarray(xforms, np.float64)
        v = np.concatenate([v @ m[:, :3].T + m[:, 3] for m in x])
    if model is not None:
        m = np.asarray(model, np.float64).reshape(4, 4).T     # column-major storage
        v = v @ m[:3, :3].T + m[:3, 3]
    return v


def checker64():
    """a 64 x 64 checker of one-texel cells"""
    return TS.checker_image(64)


def write_mip_room(directory):
    """texture_scenes.write_textured_room with images large enough for its walls to be minified: 64 x 64 and 33 x 17"""
    room = TS.write_textured_room(directory)
    rng = np.random.default_rng(43)
    TS.write_ppm(os.path.join(directory, "brick.ppm"), rng.integers(40, 256, (64, 64, 3), dtype=np.uint8))
    TS.write_ppm(os.path.join(directory, "tiles.ppm"), rng.integers(0, 256, (17, 33, 3), dtype=np.uint8))
    return room
