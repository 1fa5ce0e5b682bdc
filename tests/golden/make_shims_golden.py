"""Records tests/golden/reference_shims.json: what the reference's own nerf/{encoding,network_grid,renderer}.py ask of the three native
surfaces that customnerf_amd/dropin stands in for (raymarching, gridencoder, tinycudann).  tests/test_reference_on_shims.py checks the
shims against this record, so the suite needs no reference tree.

Run once where a checkout of the reference exists:

    CUSTOMNERF_REFERENCE=<path of the reference checkout> python tests/golden/make_shims_golden.py

Nothing of the reference's source is stored: the record holds, per NeRFNetwork constructor variant, the arguments the constructor passed
to GridEncoder / tcnn.Network and the resulting state-dict layout and optimiser groups; per call site of the native surfaces, its file,
line, callee, positional count and keyword names (an AST walk); and the GridEncoder arguments of get_encoder('hashgrid' | 'tiledgrid')."""
import ast
import json
import os
import sys
import types
import warnings

warnings.filterwarnings("ignore")
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("CUSTOMNERF_REFERENCE", "")
OUT = os.path.join(ROOT, "tests", "golden", "reference_shims.json")

# the same variants and encoder calls as tests/test_reference_on_shims.py
VARIANTS = [dict(), dict(cuda_ray=True), dict(train_conf=0), dict(detach_mask_from_field=True), dict(mask_no_dir=True),
            dict(keyword2="x", detach_mask_from_field=True)]
ENCODERS = [("hashgrid", "hash"), ("tiledgrid", "tiled")]
ENCODER_KW = dict(input_dim=3, log2_hashmap_size=19, desired_resolution=2048)


def main():
    if not os.path.isdir(os.path.join(REF, "nerf")):
        raise SystemExit("set CUSTOMNERF_REFERENCE to the reference checkout (the directory holding nerf/)")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "customnerf_amd", "dropin"))
    for name in ("trimesh", "plyfile", "skimage", "skimage.measure"):      # third-party modules the image lacks; none is on the path recorded
        sys.modules[name] = types.ModuleType(name)
    sys.modules["skimage"].measure = sys.modules["skimage.measure"]

    class _TT:
        def __class_getitem__(cls, item):
            return cls
    sys.modules["torchtyping"] = types.ModuleType("torchtyping")
    sys.modules["torchtyping"].TensorType = _TT
    sys.path.append(REF)                                                    # after the shims: only `nerf.*` comes from the reference
    import torch  # noqa: F401
    import gridencoder
    import raymarching
    import tinycudann as tcnn
    import nerf.encoding as ref_enc
    import nerf.network_grid as ref_ng
    import nerf.renderer as ref_rd
    assert ref_ng.__file__.startswith(REF) and ref_rd.__file__.startswith(REF)
    from customnerf_amd import scene as sc

    calls = []

    def recording(cls, label):
        init = cls.__init__

        def wrapped(self, *a, **k):
            calls.append([label, list(a), k])
            return init(self, *a, **k)
        return init, wrapped

    saved = {}
    for cls, label in ((gridencoder.GridEncoder, "GridEncoder"), (tcnn.Network, "tcnn.Network")):
        saved[cls], cls.__init__ = recording(cls, label)

    rec = {"variants": [], "call_sites": [], "encoders": []}
    try:
        for kw in VARIANTS:
            calls.clear()
            opt = sc.make_opt(grid_type="tiledgrid", log2_hashmap_size=21, desired_resolution=8192, **kw)
            devnull, old = open(os.devnull, "w"), sys.stdout
            sys.stdout = devnull                                            # the reference prints from its constructor
            try:
                theirs = ref_ng.NeRFNetwork(opt)
            finally:
                sys.stdout = old
            rec["variants"].append({
                "kw": kw,
                "constructor_calls": [list(c) for c in calls],
                "state": {k: [list(v.shape), str(v.dtype)] for k, v in theirs.state_dict().items()},
                "pos_en_dim": int(theirs.pos_en_dim),
                "embeddings_shape": list(theirs.pos_en.embeddings.shape),
                "param_groups": [[len(list(g["params"])), g["lr"]] for g in theirs.get_params(5e-4)],
            })
            del theirs
        for enc_name, gt in ENCODERS:
            calls.clear()
            e, dim = ref_enc.get_encoder(enc_name, **ENCODER_KW)
            assert len(calls) == 1 and calls[0][0] == "GridEncoder"
            rec["encoders"].append({"encoding": enc_name, "gridtype": gt, "dim": int(dim), "args": calls[0][1], "kwargs": calls[0][2]})
    finally:
        for cls, init in saved.items():
            cls.__init__ = init

    targets = ("raymarching", "tcnn")
    for path in (ref_rd.__file__, ref_ng.__file__, ref_enc.__file__):
        tree = ast.parse(open(path).read())
        for node in ast.walk(tree):
            if not isinstance(node, ast.Call):
                continue
            f = node.func
            if isinstance(f, ast.Attribute) and isinstance(f.value, ast.Name) and f.value.id in targets:
                label = f"{f.value.id}.{f.attr}"
            elif isinstance(f, ast.Name) and f.id == "GridEncoder":
                label = "GridEncoder"
            else:
                continue
            starred = any(isinstance(a, ast.Starred) for a in node.args) or any(k.arg is None for k in node.keywords)
            rec["call_sites"].append({"where": f"nerf/{os.path.basename(path)}:{node.lineno}", "callee": label, "n_positional": len(node.args),
                                      "keywords": [k.arg for k in node.keywords if k.arg is not None], "starred": starred})
    assert raymarching and rec["call_sites"]
    with open(OUT, "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"wrote {OUT}: {len(rec['variants'])} constructor variants, {len(rec['call_sites'])} call sites, {len(rec['encoders'])} encoders")


if __name__ == "__main__":
    main()
