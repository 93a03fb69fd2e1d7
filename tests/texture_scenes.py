"""Scenes, atlases and the numpy restatement of the albedo-texture sampler (csrc/texture.hpp) for test_textures_*.py.

The restatement follows the arithmetic as include/rtpt.h and texture.hpp state it, one numpy float32 operation per device
operation (numpy never fuses; the only fused operations of the device path are the two fmas of the uv interpolation, done
here in float64 — the product of two binary32 values is exact in binary64 — and rounded once)."""
import numpy as np

F32 = np.float32
NEAREST = 1                      # RTPT_TEX_NEAREST
TEX_SIZES = ((1, 1), (2, 2), (3, 5), (8, 8))   # (width, height)


# ------------------------------------------------------------------------------------------------ the sampler in numpy
def fma32(a, b, c):
    """fmaf for float32 arrays: a * b is exact in float64; the sum is rounded to float64 and then to float32 (two roundings:
    it can differ from a true fma in the last bit where the float64 sum lands on a float32 tie — good for values worked out
    by hand and for tolerances, not for bit comparisons with the device)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def interp_uv(b0, b1, b2, c0, c1, c2):
    """uv = fmaf(b2, uv2, fmaf(b1, uv1, b0 * uv0)), per component"""
    b0, b1, b2, c0, c1, c2 = (np.asarray(v, F32) for v in (b0, b1, b2, c0, c1, c2))
    return fma32(b2, c2, fma32(b1, c1, (b0 * c0).astype(F32)))


def wrap01(u):
    u = np.asarray(u, F32)
    return (u - np.floor(u)).astype(F32)


def _taps(s, n):
    x = ((s * F32(n)).astype(F32) - F32(0.5)).astype(F32)
    x0 = np.floor(x)
    f = (x - x0).astype(F32)
    k = x0.astype(np.int64)
    return k % n, (k + 1) % n, f


def _lerp(a, b, f):
    return (a + (f[:, None] * (b - a).astype(F32)).astype(F32)).astype(F32)


def sample(texels, desc, uv):
    """[n, 4] float32: texture `desc` = (width, height, first_texel, flags) of the atlas `texels` [m, 4] at uv [n, 2]"""
    W, H, first, flags = (int(v) for v in desc)
    uv = np.asarray(uv, F32).reshape(-1, 2)
    t = np.asarray(texels, F32).reshape(-1, 4)[first:first + W * H].reshape(H, W, 4)
    su, sv = wrap01(uv[:, 0]), wrap01(uv[:, 1])
    if flags & NEAREST:
        i = np.minimum(np.floor((su * F32(W)).astype(F32)).astype(np.int64), W - 1)
        j = np.minimum(np.floor((sv * F32(H)).astype(F32)).astype(np.int64), H - 1)
        return t[j, i]
    i0, i1, fx = _taps(su, W)
    j0, j1, fy = _taps(sv, H)
    top = _lerp(t[j0, i0], t[j0, i1], fx)
    bot = _lerp(t[j1, i0], t[j1, i1], fx)
    return _lerp(top, bot, fy)


# ------------------------------------------------------------------------------------------------ atlases
def atlas(images, flags=0, pad=3):
    """(textures [n, 4] u32, texels [m, 4] f32): the images ([H, W, 4]) behind each other with `pad` texels of a sentinel
    (-1000) in front of every one, so that every texture starts at a non-zero offset and a read beyond a rectangle shows"""
    desc, parts, first = [], [], 0
    for im in images:
        im = np.asarray(im, F32)
        h, w = im.shape[:2]
        parts.append(np.full((pad, 4), -1000.0, F32))
        first += pad
        desc.append((w, h, first, flags))
        parts.append(im.reshape(-1, 4))
        first += w * h
    return np.array(desc, np.uint32).reshape(-1, 4), np.concatenate(parts)


def distinct_image(w, h, seed):
    """every channel of every texel a different value in (0, 1)"""
    n = w * h * 4
    v = (np.arange(n, dtype=np.float64) * 0.61803398875 + 0.1 * seed + 0.05) % 1.0
    return (0.02 + 0.96 * v).astype(F32).reshape(h, w, 4)


def four_sizes(flags=0):
    """one texture of each of TEX_SIZES, distinct values per texel"""
    return atlas([distinct_image(w, h, k + 1) for k, (w, h) in enumerate(TEX_SIZES)], flags)


def constant_image(w, h, rgb):
    im = np.ones((h, w, 4), F32)
    im[..., :3] = np.asarray(rgb, F32)
    return im


def ones_atlas(flags=0):
    return atlas([np.ones((h, w, 4), F32) for w, h in TEX_SIZES], flags)


def constants_atlas(colours, flags=0):
    """texture p = a constant image of colours[p], the sizes of TEX_SIZES in turn"""
    return atlas([constant_image(*TEX_SIZES[p % len(TEX_SIZES)], c) for p, c in enumerate(colours)], flags)


def random_uv(n_tris, seed, lo=-2.5, hi=3.5):
    return np.random.default_rng(seed).uniform(lo, hi, (n_tris, 6)).astype(F32)


def sampler_uvs():
    """the uv set of the sampler parity test: texel centres and exact texel edges of every size, the special values, and
    4096 seeded random pairs in [-3, 3]"""
    vals = [0.0, 1.0, -0.0, -1e-9, 1.5, -1.5, 1e6, -1e6]
    for n in sorted({d for wh in TEX_SIZES for d in wh}):
        vals += [(k + 0.5) / n for k in range(n)] + [k / n for k in range(n + 1)] + [-(k / n) for k in range(1, n + 1)]
    vals = np.array(vals, F32)
    grid = np.stack(np.meshgrid(vals, vals), -1).reshape(-1, 2)
    rnd = np.random.default_rng(7).uniform(-3.0, 3.0, (4096, 2)).astype(F32)
    return np.concatenate([grid, rnd]).astype(F32)


# ------------------------------------------------------------------------------------------------ the quad of the geometry test
QUAD_CAM = (0.0, 1.0, 6.0)      # looks down -z at the quad's centre: K0's pixel-centre ray is K2's jitter-free ray


def quad_mesh():
    """one rectangle in the plane z = 0 under the sky, x in [-3, 3.37], y in [-2.11, 4] (it fills a 4:3 frame seen from
    QUAD_CAM and leaves sky left and right of it in a 7:1 frame).  The triangles are (0, 1, 2) and (2, 3, 0): NOT a fan pair,
    and the shared corners sit at different positions of the two records, so swapped barycentrics cannot cancel.  The odd
    extents keep the shared diagonal away from the pixel centres: with a diagonal of slope 1 through the camera's axis a
    whole row of jitter-free rays runs exactly along the shared edge, where the two triangles' edge tests (the edge is
    stated in opposite directions) need not agree and K0 and K2 resolve the tie differently."""
    xyz = np.array([[-3, -2.11, 0], [3.37, -2.11, 0], [3.37, 4, 0], [-3, 4, 0]], F32)
    idx = np.array([[0, 1, 2], [2, 3, 0]], np.uint32)
    return xyz, idx


# uv = QUAD_A @ (x, y) + QUAD_C: a rotation by 25 degrees with a shear, scaled so that the quad's corners stay in [0.1, 0.9]
def _quad_map():
    th = np.deg2rad(25.0)
    a = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]) @ np.array([[1.0, 0.35], [0.0, 1.0]])
    corners = quad_mesh()[0][:, :2].astype(np.float64)
    raw = corners @ a.T
    lo, hi = raw.min(0), raw.max(0)
    scale = 0.8 / (hi - lo)
    return a * scale[:, None], 0.1 - lo * scale


QUAD_A, QUAD_C = _quad_map()


def quad_uv_of(xy):
    """float64 uv of points [..., 2] of the quad's plane"""
    return np.asarray(xy, np.float64) @ QUAD_A.T + QUAD_C


def quad_tri_uv():
    xyz, idx = quad_mesh()
    uv = quad_uv_of(xyz[:, :2])
    assert uv.min() >= 0.1 - 1e-12 and uv.max() <= 0.9 + 1e-12
    return uv[idx].reshape(-1, 6).astype(F32)


def ramp_image(n=8):
    """texel (i, j) = ((i + 0.5) / n, (j + 0.5) / n, 0): bilinear sampling returns (u, v) inside [0.5 / n, 1 - 0.5 / n]"""
    c = ((np.arange(n) + 0.5) / n).astype(F32)
    im = np.zeros((n, n, 4), F32)
    im[..., 0] = c[None, :]
    im[..., 1] = c[:, None]
    im[..., 3] = 1.0
    return im


def checker_image(n=8, a=(0.9, 0.15, 0.1), b=(0.1, 0.2, 0.9)):
    ij = np.add.outer(np.arange(n), np.arange(n)) & 1
    im = np.ones((n, n, 4), F32)
    im[..., :3] = np.where(ij[..., None] == 0, np.asarray(a, F32), np.asarray(b, F32))
    return im


# ------------------------------------------------------------------------------------------------ files for the loader / hosts
def write_ppm(path, rgb8):
    """binary P6 from [H, W, 3] uint8, top row first"""
    rgb8 = np.ascontiguousarray(rgb8, np.uint8)
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (rgb8.shape[1], rgb8.shape[0]))
        f.write(rgb8.tobytes())


def write_pfm(path, rgb):
    """colour PFM (little endian) from [H, W, 3] float32, BOTTOM row first (the format's order)"""
    rgb = np.ascontiguousarray(rgb, "<f4")
    with open(path, "wb") as f:
        f.write(b"PF\n%d %d\n-1.0\n" % (rgb.shape[1], rgb.shape[0]))
        f.write(rgb.tobytes())


def write_textured_room(directory):
    """room.obj + room.mtl + two P6 images in `directory`: a back wall and a floor (quads with texture coordinates reaching
    outside [0, 1], so the images repeat), a tilted panel without texture coordinates and a small emissive quad.  Returns the
    OBJ's path.  Seen from the hosts' default camera at (-0.001, 1, 6)."""
    import os
    rng = np.random.default_rng(42)
    write_ppm(os.path.join(directory, "brick.ppm"), rng.integers(40, 256, (4, 4, 3), dtype=np.uint8))
    write_ppm(os.path.join(directory, "tiles.ppm"), rng.integers(0, 256, (5, 3, 3), dtype=np.uint8))
    with open(os.path.join(directory, "room.mtl"), "w") as f:
        f.write("newmtl brick\nKd 0.9 0.8 0.7\nmap_Kd brick.ppm\n"
                "newmtl tiles\nKd 1 1 1\nmap_Kd tiles.ppm\n"
                "newmtl panel\nKd 0.2 0.6 0.3\n"
                "newmtl lamp\nKd 0 0 0\nKe 4 3 2\n")
    with open(os.path.join(directory, "room.obj"), "w") as f:
        f.write("mtllib room.mtl\n"
                "v -2 -0.2 -1\nv 2 -0.2 -1\nv 2 2.4 -1\nv -2 2.4 -1\n"        # back wall
                "v -2 -0.2 3\nv 2 -0.2 3\n"                                   # floor front edge
                "v -0.6 0.3 0.5\nv 0.5 0.2 0.2\nv 0.6 1.3 0.0\nv -0.5 1.4 0.4\n"   # panel
                "v 1.0 1.8 -0.9\nv 1.5 1.8 -0.9\nv 1.5 2.2 -0.9\nv 1.0 2.2 -0.9\n"   # lamp
                "vt -0.5 -0.25\nvt 2.5 -0.25\nvt 2.5 1.75\nvt -0.5 1.75\n"
                "vt 0 0\nvt 3 0\nvt 3.5 2\nvt 0.5 2\n"
                "usemtl brick\nf 1/1 2/2 3/3 4/4\n"
                "usemtl tiles\nf 5/5 6/6 2/7 1/8\n"
                "usemtl panel\nf 7 8 9 10\n"
                "usemtl lamp\nf 11//1 12//1 13//1 14//1\n")
    return os.path.join(directory, "room.obj")
