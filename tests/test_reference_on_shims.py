"""Reference-on-shims conformance (CPU): what the reference's OWN nerf/{encoding,network_grid,renderer}.py ask of the
native surfaces, recorded in tests/golden/reference_shims.json (tests/golden/make_shims_golden.py: the reference's modules imported
unmodified with customnerf_amd/dropin first on sys.path), replayed against the shims — `import raymarching`, `from gridencoder import
GridEncoder` and `import tinycudann as tcnn` resolve to this package, and:

  * every GridEncoder / tcnn.Network constructor call that `NeRFNetwork(opt)` (network_grid.py:70-139) made, for cuda_ray on and off and for
    every rgb-head variant, binds and constructs on the shims;
  * the reference model's state-dict keys / shapes / dtypes equal the product class's for the same geometry (checkpoints interchange);
  * every `raymarching.*` / `GridEncoder(...)` / `tcnn.Network(...)` call site in those three files (AST walk; renderer.py:297, 612-688,
    1680, 1709 among them) binds against the shim's signature — positional count and keyword names;
  * the encoders the reference builds through its get_encoder (encoding.py:52-71) come out of the shim with the reference's geometry.

The record holds data only (arguments, names, shapes); no reference source is stored or read."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "tests", "golden", "reference_shims.json")

WORKER = r'''
import inspect, json, os, sys, warnings
warnings.filterwarnings("ignore")
ROOT, RECORD = %r, %r
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "customnerf_amd", "dropin"))       # the names the reference imports: raymarching / gridencoder / tinycudann
import torch
import raymarching, gridencoder, tinycudann as tcnn
assert raymarching.__file__.startswith(ROOT) and gridencoder.__file__.startswith(ROOT) and tcnn.__file__.startswith(ROOT)
from customnerf_amd import scene as sc
from customnerf_amd.nerf.network_grid import NeRFNetwork as Ours
rec = json.load(open(RECORD))
surfaces = {"GridEncoder": gridencoder.GridEncoder, "tcnn.Network": tcnn.Network}

# ---- 1. constructor + state dict, every head variant the reference's __init__ branches on (network_grid.py:112-139)
assert len(rec["variants"]) == 6
built = set()
for v in rec["variants"]:
    kw = v["kw"]
    assert v["pos_en_dim"] == 32 and v["embeddings_shape"] == [23967296, 2]                        # SURVEY §8: the bear table
    for label, args, kwargs in v["constructor_calls"]:
        cls = surfaces[label]
        sig = inspect.signature(cls.__init__)
        try:
            sig.bind(None, *args, **kwargs)
        except TypeError as e:
            raise AssertionError(f"{kw}: {label}{tuple(args)} {kwargs} does not bind against {sig}: {e}")
        key = json.dumps([label, args, kwargs], sort_keys=True)
        if key not in built:
            m = cls(*args, **kwargs)
            built.add(key)
            if label == "GridEncoder":
                assert list(m.embeddings.shape) == v["embeddings_shape"] and m.output_dim == v["pos_en_dim"], kw
            del m
    assert sum(c[0] == "GridEncoder" for c in v["constructor_calls"]) == 1, kw
    opt = sc.make_opt(grid_type="tiledgrid", log2_hashmap_size=21, desired_resolution=8192, **kw)
    ours = Ours(opt)
    a = {k: (tuple(s), d) for k, (s, d) in v["state"].items()}
    b = {k: (tuple(t.shape), str(t.dtype)) for k, t in ours.state_dict().items()}
    assert a == b, (kw, sorted(set(a.items()) ^ set(b.items())))
    assert ours.pos_en_dim == v["pos_en_dim"] and list(ours.pos_en.embeddings.shape) == v["embeddings_shape"], kw
    pb = [[len(list(g["params"])), g["lr"]] for g in ours.get_params(5e-4)]                        # optimiser groups: grid lr x10 (network_grid.py:196-206)
    assert pb == v["param_groups"], (kw, pb, v["param_groups"])
    del ours
print("constructors ok")

# ---- 2. every call site of the three native surfaces binds against the shim
targets = {"raymarching": raymarching, "tcnn": tcnn}
n_sites = {}
for site in rec["call_sites"]:
    label = site["callee"]
    if label == "GridEncoder":
        fn = gridencoder.GridEncoder
    else:
        mod, attr = label.split(".")
        assert hasattr(targets[mod], attr), f"{site['where']}: {label} missing from the shim"
        fn = getattr(targets[mod], attr)
    if site["starred"]:
        continue
    sig = inspect.signature(fn.__init__) if inspect.isclass(fn) else inspect.signature(fn)
    args = ([None] if inspect.isclass(fn) else []) + [None] * site["n_positional"]
    try:
        sig.bind(*args, **{k: None for k in site["keywords"]})
    except TypeError as e:
        raise AssertionError(f"{site['where']}: {label} call does not bind against {sig}: {e}")
    n_sites[label] = n_sites.get(label, 0) + 1
for need in ("raymarching.near_far_from_aabb", "raymarching.march_rays_train", "raymarching.composite_rays_train", "raymarching.march_rays",
             "raymarching.composite_rays", "raymarching.morton3D", "raymarching.packbits", "tcnn.Network", "GridEncoder"):
    assert n_sites.get(need, 0) >= 1, (need, n_sites)
print("call sites ok", sorted(n_sites.items()))

# ---- 3. the encoder the reference builds through ITS get_encoder is the product's, with the reference's geometry (encoding.py:52-71)
assert [(e["encoding"], e["gridtype"]) for e in rec["encoders"]] == [("hashgrid", "hash"), ("tiledgrid", "tiled")]
for enc in rec["encoders"]:
    e = gridencoder.GridEncoder(*enc["args"], **enc["kwargs"])
    dim = e.output_dim
    assert dim == enc["dim"] == 32 and e.gridtype == enc["gridtype"] and e.embeddings.shape[0] == int(e.offsets[-1]) and e.n_params == e.embeddings.numel()
print("encoders ok")
'''


def test_reference_modules_run_on_the_shims(tmp_path):
    script = tmp_path / "conformance.py"
    script.write_text(WORKER % (ROOT, RECORD))
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    assert "constructors ok" in out.stdout and "call sites ok" in out.stdout and "encoders ok" in out.stdout
