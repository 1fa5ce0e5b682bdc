"""A glTF 2.0 binary read back without any library, for the tests of mesh.write_glb (tests/test_mesh_glb_host.py on the CPU,
tests/test_gpu_mesh_tangent.py on the GPU).  A plain module: neither test file imports the other."""
import json
import struct
import zlib

import numpy as np

f32 = np.float32
COMPONENTS = {5121: ("u1", 1), 5123: ("<u2", 2), 5125: ("<u4", 4), 5126: ("<f4", 4)}
WIDTH = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4}


def parse_glb(path):
    """(the JSON document, the BIN chunk) after checking the container: magic, version 2, the total length, a JSON chunk padded with
    spaces, then a BIN chunk padded with zeros, both multiples of 4"""
    data = open(path, "rb").read()
    magic, version, total = struct.unpack_from("<4sII", data, 0)
    assert magic == b"glTF" and version == 2 and total == len(data) and total % 4 == 0
    n, kind = struct.unpack_from("<I4s", data, 12)
    assert kind == b"JSON" and n % 4 == 0
    js = data[20:20 + n]
    assert js.rstrip(b" ") == js.strip() and js[:1] == b"{"                    # padded with trailing spaces only
    doc = json.loads(js.decode("utf-8"))
    o = 20 + n
    m, kind = struct.unpack_from("<I4s", data, o)
    assert kind == b"BIN\0" and m % 4 == 0 and o + 8 + m == total
    blob = data[o + 8:]
    assert doc["buffers"] == [{"byteLength": m}] or (doc["buffers"][0]["byteLength"] <= m and m - doc["buffers"][0]["byteLength"] < 4)
    return doc, blob


def read_accessor(doc, blob, i):
    a = doc["accessors"][i]
    bv = doc["bufferViews"][a["bufferView"]]
    dt, size = COMPONENTS[a["componentType"]]
    w = WIDTH[a["type"]]
    assert bv["byteOffset"] % 4 == 0 and bv["byteLength"] == a["count"] * w * size and bv["byteOffset"] + bv["byteLength"] <= len(blob)
    return np.frombuffer(blob, dt, a["count"] * w, bv["byteOffset"]).reshape(a["count"], w) if w > 1 else \
        np.frombuffer(blob, dt, a["count"], bv["byteOffset"])


def read_png_bytes(data):
    """[H, W, 3] uint8 of an 8-bit RGB PNG whose rows all use filter 0"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    o, idat, shape = 8, b"", None
    while o < len(data):
        n, tag = struct.unpack_from(">I4s", data, o)
        body = data[o + 8:o + 8 + n]
        assert struct.unpack_from(">I", data, o + 8 + n)[0] == zlib.crc32(tag + body) & 0xffffffff
        if tag == b"IHDR":
            W, H, depth, colour, comp, filt, inter = struct.unpack(">IIBBBBB", body)
            assert (depth, colour, comp, filt, inter) == (8, 2, 0, 0, 0)
            shape = (H, W)
        elif tag == b"IDAT":
            idat += body
        o += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(shape[0], 1 + 3 * shape[1])
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(shape[0], shape[1], 3)


def image_bytes(doc, blob, i):
    img = doc["images"][i]
    assert img["mimeType"] == "image/png"
    bv = doc["bufferViews"][img["bufferView"]]
    assert bv["byteOffset"] % 4 == 0 and "target" not in bv
    return blob[bv["byteOffset"]:bv["byteOffset"] + bv["byteLength"]]
