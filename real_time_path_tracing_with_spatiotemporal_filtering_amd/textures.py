"""Albedo textures for the Python host: image files (binary PPM and PFM only), the atlas rtpt_scene_set_textures takes, and
what an OBJ + MTL pair says about them (`vt`, `map_Kd`).  Host-side preparation only; sampling is csrc/texture.hpp."""
from __future__ import annotations

import os
from typing import NamedTuple

import numpy as np

from . import abi


def _tokens(data: bytes, n: int):
    """the first n whitespace-separated header tokens of a PNM / PFM file ('#' comments skipped) and the offset of the
    byte behind the single whitespace that ends the last one"""
    out, i = [], 0
    while len(out) < n:
        while i < len(data) and data[i:i + 1].isspace():
            i += 1
        if data[i:i + 1] == b"#":
            while i < len(data) and data[i:i + 1] != b"\n":
                i += 1
            continue
        j = i
        while j < len(data) and not data[j:j + 1].isspace():
            j += 1
        if j == i:
            raise ValueError("truncated image header")
        out.append(data[i:j])
        i = j
    return out, i + 1


def load_image(path: str) -> np.ndarray:
    """[H, W, 4] float32 RGBA (alpha 1), linear, row 0 = the BOTTOM row of the picture (OBJ's v = 0).  Binary PPM (`P6`,
    maxval <= 255: byte / 255.0f) and PFM (`PF` colour, `Pf` grey; either byte order) only — there is no PNG / JPEG decoder."""
    with open(path, "rb") as f:
        data = f.read()
    magic = data[:2]
    if magic == b"P6":
        (_, w, h, maxval), off = _tokens(data, 4)
        w, h, maxval = int(w), int(h), int(maxval)
        if not 0 < maxval <= 255:
            raise ValueError(f"{path}: only 8-bit P6 images are supported (maxval {maxval})")
        px = np.frombuffer(data, np.uint8, w * h * 3, off).reshape(h, w, 3)
        rgb = px.astype(np.float32) / np.float32(255.0)
        rgb = rgb[::-1]  # PPM stores the top row first
    elif magic in (b"PF", b"Pf"):
        (_, w, h, scale), off = _tokens(data, 4)
        w, h, ch = int(w), int(h), 3 if magic == b"PF" else 1
        dt = np.dtype("<f4") if float(scale) < 0 else np.dtype(">f4")
        rgb = np.frombuffer(data, dt, w * h * ch, off).reshape(h, w, ch).astype(np.float32)  # PFM stores the bottom row first
        if ch == 1:
            rgb = np.repeat(rgb, 3, axis=2)
    else:
        raise ValueError(f"{path}: unsupported image format {magic!r} — textures are binary PPM (P6) or PFM files; "
                         "convert other formats first")
    out = np.ones((h, w, 4), np.float32)
    out[..., :3] = rgb
    return out


def build_atlas(images, nearest=False, mips=False):
    """(textures [n, 4] u32, texels [m, 4] f32) for rtpt_scene_set_textures: the images ([H, W, 4] f32, row 0 = v 0) one
    after the other; `mips`: every texture gets RTPT_TEX_MIPMAP (the library generates the chains on the device)"""
    desc, parts, first = [], [], 0
    flags = (abi.TEX_NEAREST if nearest else 0) | (abi.TEX_MIPMAP if mips else 0)
    for im in images:
        im = np.ascontiguousarray(im, np.float32)
        h, w = im.shape[:2]
        desc.append((w, h, first, flags))
        parts.append(im.reshape(-1, 4))
        first += w * h
    return np.array(desc, np.uint32).reshape(-1, 4), np.concatenate(parts) if parts else np.zeros((0, 4), np.float32)


class ObjTextures(NamedTuple):
    tri_material: np.ndarray | None   # abi.load_obj_materials
    materials: np.ndarray | None
    tri_uv: np.ndarray | None         # what Context.set_textures takes; None: no material names a map
    tri_texture: np.ndarray | None
    textures: np.ndarray | None
    texels: np.ndarray | None


def load_obj_textures(path: str, nearest=False, mips=False) -> ObjTextures:
    """the material library of an OBJ with its `map_Kd` images (looked up next to the OBJ) as one atlas"""
    tri_material, materials = abi.load_obj_materials(path)
    maps = abi.load_obj_map_kd(path)
    if tri_material is None or not maps or not any(maps):
        return ObjTextures(tri_material, materials, None, None, None, None)
    files = sorted({m for m in maps if m})
    images = [load_image(os.path.join(os.path.dirname(path), f)) for f in files]
    of_material = np.array([files.index(m) + 1 if m else 0 for m in maps], np.uint32)
    textures, texels = build_atlas(images, nearest, mips)
    return ObjTextures(tri_material, materials, abi.load_obj_texcoords(path), of_material[tri_material], textures, texels)
