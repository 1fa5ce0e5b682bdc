"""CPU: mesh.write_glb writes a glTF 2.0 binary that this file parses back by itself (header, chunks, accessors, bufferViews, images,
material), mesh.png_bytes / write_png still write the bytes they always did, and the arguments write_glb refuses."""
import os
import struct
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from glb_testlib import image_bytes, parse_glb, read_accessor, read_png_bytes  # noqa: E402

f32 = np.float32


def sample(W=7, F=5, seed=0):
    rng = np.random.default_rng(seed)
    pos = rng.standard_normal((W, 3)).astype(f32)
    nrm = rng.standard_normal((W, 3)).astype(f32)
    uv = rng.random((W, 2)).astype(f32)
    tan = np.concatenate([rng.standard_normal((W, 3)), np.sign(rng.standard_normal((W, 1)))], 1).astype(f32)
    idx = rng.integers(0, W, (F, 3)).astype(np.uint32)
    tex = rng.integers(0, 256, (8, 8, 3)).astype(np.uint8)
    nm = rng.integers(0, 256, (8, 8, 3)).astype(np.uint8)
    col = rng.integers(0, 256, (W, 3)).astype(np.uint8)
    return pos, idx, nrm, uv, tan, tex, nm, col


def test_full_file(tmp_path):
    from customnerf_amd import mesh
    pos, idx, nrm, uv, tan, tex, nm, col = sample()
    W, F = len(pos), len(idx)
    path = str(tmp_path / "m.glb")
    mesh.write_glb(path, pos, idx, normals=nrm, uvs=uv, tangents=tan, colors=col, texture=tex, normal_map=nm)
    doc, blob = parse_glb(path)
    assert doc["asset"]["version"] == "2.0" and doc["scene"] == 0 and doc["scenes"][0]["nodes"] == [0] and doc["nodes"][0]["mesh"] == 0
    prim, = doc["meshes"][0]["primitives"]
    assert prim["mode"] == 4 and prim["material"] == 0
    att = prim["attributes"]
    assert set(att) == {"POSITION", "NORMAL", "TEXCOORD_0", "TANGENT", "COLOR_0"}
    want = {prim["indices"]: (3 * F, "SCALAR", 5125, 34963), att["POSITION"]: (W, "VEC3", 5126, 34962),
            att["NORMAL"]: (W, "VEC3", 5126, 34962), att["TEXCOORD_0"]: (W, "VEC2", 5126, 34962), att["TANGENT"]: (W, "VEC4", 5126, 34962),
            att["COLOR_0"]: (W, "VEC4", 5121, 34962)}
    assert len(want) == len(doc["accessors"]) == 6
    for i, (count, kind, ctype, target) in want.items():
        a = doc["accessors"][i]
        assert (a["count"], a["type"], a["componentType"]) == (count, kind, ctype), i
        assert doc["bufferViews"][a["bufferView"]]["target"] == target
        assert ("min" in a) == ("max" in a) == (i == att["POSITION"])
        assert a.get("normalized", False) == (i == att["COLOR_0"])
    a = doc["accessors"][att["POSITION"]]
    assert a["min"] == pos.min(0).astype(np.float64).tolist() and a["max"] == pos.max(0).astype(np.float64).tolist()
    # views: inside the buffer, 4-byte aligned, not overlapping, in order
    end = 0
    for bv in doc["bufferViews"]:
        assert bv["buffer"] == 0 and bv["byteOffset"] % 4 == 0 and bv["byteOffset"] >= end
        end = bv["byteOffset"] + bv["byteLength"]
    assert end <= len(blob) and doc["buffers"][0]["byteLength"] == len(blob)
    assert read_accessor(doc, blob, prim["indices"]).tobytes() == idx.astype("<u4").tobytes()
    assert read_accessor(doc, blob, att["POSITION"]).tobytes() == pos.tobytes()
    assert read_accessor(doc, blob, att["NORMAL"]).tobytes() == nrm.tobytes()
    assert read_accessor(doc, blob, att["TANGENT"]).tobytes() == tan.tobytes()
    assert read_accessor(doc, blob, att["TEXCOORD_0"]).tobytes() == uv.tobytes()
    rgba = read_accessor(doc, blob, att["COLOR_0"])
    assert (rgba[:, :3] == col).all() and (rgba[:, 3] == 255).all()
    # the material and both images
    mat, = doc["materials"]
    pbr = mat["pbrMetallicRoughness"]
    assert pbr["metallicFactor"] == 0 and pbr["roughnessFactor"] == 1
    t_img = doc["textures"][pbr["baseColorTexture"]["index"]]["source"]
    n_img = doc["textures"][mat["normalTexture"]["index"]]["source"]
    assert t_img != n_img and len(doc["images"]) == 2
    np.testing.assert_array_equal(read_png_bytes(image_bytes(doc, blob, t_img)), tex)
    np.testing.assert_array_equal(read_png_bytes(image_bytes(doc, blob, n_img)), nm)
    assert image_bytes(doc, blob, t_img) == mesh.png_bytes(tex)
    # with a normal map the material is lit
    assert "extensionsUsed" not in doc and "extensions" not in mat


def test_texcoord_is_flipped_by_the_caller(tmp_path):
    """TEXCOORD_0 holds (u, 1 - v) of the project's UVs: the restatement's vertex buffers, written and read back"""
    from customnerf_amd import mesh
    import tangent_restatement as TR
    import tangent_testlib as TL
    v, f, uv, n, _ = TL.hand_soup()
    g = TR.vertices(v, f, uv, n)
    path = str(tmp_path / "soup.glb")
    mesh.write_glb(path, g['positions'], g['indices'], normals=g['normals'], uvs=g['uvs'], tangents=g['tangents'])
    doc, blob = parse_glb(path)
    att = doc["meshes"][0]["primitives"][0]["attributes"]
    got = read_accessor(doc, blob, att["TEXCOORD_0"])
    cv, vc = TR.weld(f, uv)
    flat = uv.reshape(-1, 2)
    assert got.tobytes() == np.stack([flat[vc, 0], f32(1) - flat[vc, 1]], -1).astype(f32).tobytes()
    assert read_accessor(doc, blob, doc["meshes"][0]["primitives"][0]["indices"]).reshape(-1, 3).tolist() == cv.tolist()
    assert doc["accessors"][att["POSITION"]]["count"] == len(vc)


@pytest.mark.parametrize("normal_map,unlit,want", [(False, None, True), (True, None, False), (False, False, False), (True, True, True),
                                                   (False, True, True), (True, False, False)])
def test_unlit(tmp_path, normal_map, unlit, want):
    from customnerf_amd import mesh
    pos, idx, nrm, uv, tan, tex, nm, col = sample(seed=1)
    path = str(tmp_path / "u.glb")
    mesh.write_glb(path, pos, idx, normals=nrm, uvs=uv, tangents=tan, texture=tex, normal_map=nm if normal_map else None, unlit=unlit)
    doc, _ = parse_glb(path)
    mat, = doc["materials"]
    assert (doc.get("extensionsUsed") == ["KHR_materials_unlit"]) == want
    assert ("KHR_materials_unlit" in mat.get("extensions", {})) == want
    assert ("normalTexture" in mat) == normal_map and len(doc["images"]) == 1 + normal_map


def test_geometry_only_and_empty(tmp_path):
    """positions and indices alone (torch tensors too), and a mesh without a vertex"""
    import torch
    from customnerf_amd import mesh
    pos, idx, nrm, *_ = sample(seed=2)
    path = str(tmp_path / "g.glb")
    mesh.write_glb(path, torch.from_numpy(pos), torch.from_numpy(idx.astype(np.int32)), normals=torch.from_numpy(nrm))
    doc, blob = parse_glb(path)
    prim, = doc["meshes"][0]["primitives"]
    assert set(prim["attributes"]) == {"POSITION", "NORMAL"} and "images" not in doc and "textures" not in doc
    assert "baseColorTexture" not in doc["materials"][0]["pbrMetallicRoughness"]
    assert doc["extensionsUsed"] == ["KHR_materials_unlit"]
    assert read_accessor(doc, blob, prim["indices"]).tobytes() == idx.astype("<u4").tobytes()
    mesh.write_glb(path, np.zeros((0, 3), f32), np.zeros((0, 3), np.int32))
    doc, blob = parse_glb(path)
    assert doc["accessors"][doc["meshes"][0]["primitives"][0]["attributes"]["POSITION"]]["count"] == 0


def parent_png(image):
    """write_png as it stood before png_bytes was split out of it, restated: signature, IHDR, one IDAT of zlib level 6 over rows that
    each start with filter byte 0, IEND"""
    a = np.ascontiguousarray(image, np.uint8)
    H, W = a.shape[:2]
    raw = np.zeros((H, 1 + 3 * W), np.uint8)
    raw[:, 1:] = a.reshape(H, 3 * W)

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)

    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) + \
        chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)) + chunk(b"IEND", b"")


def test_write_png_is_unchanged(tmp_path):
    from customnerf_amd import mesh
    Y, X = np.meshgrid(np.arange(13), np.arange(21), indexing="ij")
    img = np.stack([(7 * X + 3 * Y) % 256, (X * Y) % 256, (255 - 5 * X) % 256], -1).astype(np.uint8)
    path = str(tmp_path / "a.png")
    mesh.write_png(path, img)
    data = open(path, "rb").read()
    assert data == parent_png(img) == mesh.png_bytes(img)
    np.testing.assert_array_equal(read_png_bytes(data), img)
    with pytest.raises(ValueError, match="write_png"):
        mesh.write_png(path, img[..., 0])


def test_refused_arguments(tmp_path):
    from customnerf_amd import mesh
    pos, idx, nrm, uv, tan, tex, nm, col = sample(seed=3)
    path = str(tmp_path / "bad.glb")
    W = len(pos)
    with pytest.raises(ValueError, match="normal map"):
        mesh.write_glb(path, pos, idx, normals=nrm, uvs=uv, texture=tex, normal_map=nm)                       # no tangents
    with pytest.raises(ValueError, match="normal map"):
        mesh.write_glb(path, pos, idx, normals=nrm, tangents=tan, normal_map=nm)                              # no uvs
    with pytest.raises(ValueError, match="texture"):
        mesh.write_glb(path, pos, idx, normals=nrm, texture=tex)
    for name, a in (("normals", nrm), ("uvs", uv), ("tangents", tan), ("colors", col)):
        with pytest.raises(ValueError, match=name):
            mesh.write_glb(path, pos, idx, **{name: a[:W - 1]})
    for bad in (W, -1):
        i2 = idx.astype(np.int64)
        i2[1, 2] = bad
        with pytest.raises(ValueError, match="index"):
            mesh.write_glb(path, pos, i2)
    assert not os.path.exists(path)
