"""CPU: the mesh export pipeline (customnerf_amd/nerf/mesh_export.py) up to its first launch — the public signatures NeRFRenderer keeps,
the one camera-set validator behind tsdf= and color_views=, and every refusal of extract_mesh on a model that lives on the host."""
import inspect

import numpy as np
import pytest

# str(inspect.signature(...)) of the methods as they stood before the pipeline moved out of NeRFRenderer
SIGNATURES = {
    'extract_mesh': "(self, resolution=256, threshold=None, aabb=None, chunk=2097152, part='all', view_dir=(0.0, 0.0, -1.0), color=False, min_component_faces=0, keep_largest=False, simplify=0, target_faces=0, texture=0, smooth=0, smooth_lambda=0.5, smooth_mu=-0.53, deviation=False, deviation_spacing=None, deviation_max_samples=67108864, ao=0, texture_layout='uniform', bake_from='mesh', bake_reach=None, normal_map=False, sparse=False, sparse_probe=4, tsdf=None, fill_holes=False, topology=False, color_views=None, remesh=None)",
    'save_mesh': '(self, path, **kw)',
    'render_depth': "(self, c2w, intrinsics, H, W, convention='nerfstudio', min_opacity=0.5, max_ray_batch=65536, **render_kw)",
    'render_view': "(self, c2w, intrinsics, H, W, convention='nerfstudio', min_opacity=0.5, max_ray_batch=65536, **render_kw)",
    'render_mesh': "(self, mesh, c2w, intrinsics, H, W, path=None, map='texture', **kw)",
    'density_volume': "(self, resolution=256, aabb=None, chunk=2097152, part='all', view_dir=(0.0, 0.0, -1.0))",
}

EYE = np.eye(4, dtype=np.float32)
GOOD = dict(poses=np.stack([EYE, EYE]), intrinsics=(1, 1, 2, 2), H=4, W=4)


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_public_signatures_are_pinned(name):
    from customnerf_amd.nerf.renderer import NeRFRenderer
    assert name in vars(NeRFRenderer) and vars(NeRFRenderer)[name].__doc__
    assert str(inspect.signature(getattr(NeRFRenderer, name))) == SIGNATURES[name]


def without(key):
    return {k: v for k, v in GOOD.items() if k != key}


# (fault, what the message says about it; {o} is the option's name)
CAMERA_FAULTS = [
    (without('poses'), "{o} needs ['poses']"), (without('intrinsics'), "{o} needs ['intrinsics']"),
    (without('H'), "{o} needs ['H']"), (without('W'), "{o} needs ['W']"),
    ({**GOOD, 'poses': np.zeros((0, 4, 4), np.float32)}, "{o}['poses'] holds no view"),
    ({**GOOD, 'poses': EYE}, "{o}['poses'] must be [N, 3, 4] or [N, 4, 4], got (4, 4)"),
    ({**GOOD, 'convention': 'opencv'}, "{o}['convention'] must be"),
    ({**GOOD, 'intrinsics': (1, 1, 2)}, "{o}['intrinsics'] must be (fx, fy, cx, cy), got 3 values"),
    ({**GOOD, 'colour': True}, "unknown {o} keys ['colour']"),
    ({**GOOD, 'H': 0}, "{o} needs H, W >= "), ({**GOOD, 'W': 0}, "{o} needs H, W >= "),
]


def options(kind):
    from customnerf_amd.nerf import mesh_export
    if kind == 'tsdf':
        return lambda d: mesh_export.tsdf_options(d, False, 'all', 0.25)
    return lambda d: mesh_export.color_view_options(d, None, True, 0.25)


@pytest.mark.parametrize("kind", ["tsdf", "color_views"])
def test_camera_set_validator(kind):
    from customnerf_amd.nerf import mesh_export
    opts, other = options(kind), 'color_views' if kind == 'tsdf' else 'tsdf'
    cfg = opts(GOOD)
    assert tuple(cfg['poses'].shape) == (2, 4, 4) and cfg['intrinsics'] == (1.0, 1.0, 2.0, 2.0) and (cfg['H'], cfg['W']) == (4, 4)
    assert cfg['convention'] == 'nerfstudio' and cfg['min_opacity'] == 0.5 and cfg['render'] == {}
    for fault, says in CAMERA_FAULTS:
        with pytest.raises(ValueError) as e:
            opts(fault)
        msg = str(e.value)
        assert msg.startswith("extract_mesh: ") and says.format(o=kind) in msg and other not in msg, msg
    # the two differences between the kinds: the smallest image, and whether the poses must be finite
    nan_pose = np.stack([EYE, EYE])
    nan_pose[0, 1, 1] = np.inf
    if kind == 'tsdf':
        assert opts({**GOOD, 'H': 1})['H'] == 1 and opts({**GOOD, 'W': 1})['W'] == 1
        assert not np.isfinite(opts({**GOOD, 'poses': nan_pose})['poses'].numpy()).all()
    else:
        for fault, says in (({**GOOD, 'H': 1}, "color_views needs H, W >= 2, got 1, 4"), ({**GOOD, 'W': 1}, "color_views needs H, W >= 2, got 4, 1"),
                            ({**GOOD, 'poses': nan_pose}, "color_views['poses'] holds non-finite values")):
            with pytest.raises(ValueError) as e:
                opts(fault)
            assert says in str(e.value)
    # the validator itself: the name it is given is the one it reports
    with pytest.raises(ValueError, match=r"views\['poses'\] holds no view"):
        mesh_export.camera_set({**GOOD, 'poses': GOOD['poses'][:0]}, 'views', mesh_export.TSDF_KEYS, 1, False)


TSDF = {**GOOD, 'min_opacity': 0.9}
REFUSED = [
    dict(fill_holes='all'), dict(fill_holes=2), dict(fill_holes=1.5), dict(fill_holes=True, simplify=2), dict(fill_holes=5, simplify=3),
    dict(resolution=1), dict(aabb=[0, 0, 0, 1, 1, 0]), dict(simplify=1), dict(simplify=-2), dict(target_faces=-1),
    dict(target_faces=100, simplify=2), dict(texture=-1), dict(texture_layout='atlas'), dict(smooth=-1), dict(ao=-1), dict(bake_from='field'),
    dict(normal_map='object'), dict(normal_map=True), dict(normal_map='tangent'), dict(bake_from='source', bake_reach=0.0),
    dict(bake_from='source', bake_reach=-1.0), dict(bake_from='source', bake_reach=float('nan')), dict(sparse_probe=0),
    dict(remesh='fine'), dict(remesh=True), dict(remesh=2.5), dict(remesh={}), dict(remesh=dict(resolution=16, voxel=0.1)),
    dict(remesh=dict(resolution=16, level=0.0)), dict(color_views=GOOD), dict(color_views='tsdf', color=True),
    dict(color_views='views', color=True), dict(color_views={**GOOD, 'H': 1}, color=True), dict(color_views={**GOOD, 'power': 0}, texture=64),
    dict(color_views={**GOOD, 'min_cos': 1.0}, color=True), dict(color_views={**GOOD, 'depth_tol': 0.0}, color=True),
    dict(tsdf=[TSDF]), dict(tsdf=TSDF, sparse=True), dict(tsdf=TSDF, part='fg'), dict(tsdf={**TSDF, 'trunc': 0.0}),
    dict(tsdf={**TSDF, 'depth_tol': 0.1}), dict(tsdf=without('W')), dict(tsdf={**TSDF, 'poses': EYE}), dict(part='foreground'),
    dict(part='foreground', sparse=True),
]


@pytest.fixture(scope="module")
def host_model():
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    from customnerf_amd.scene import make_opt
    return NeRFNetwork(make_opt())                                                # on the host: anything past the checks has no device to run on


@pytest.mark.parametrize("kw", REFUSED, ids=lambda kw: "-".join(kw))
def test_every_refusal_comes_before_any_launch(host_model, kw):
    with pytest.raises(ValueError, match="^extract_mesh: "):
        host_model.extract_mesh(**{'resolution': 8, **kw})


def test_valid_options_reach_the_device(host_model):
    """the counterpart: with nothing to refuse, a host model fails at its first device call, and not with a ValueError"""
    from customnerf_amd.nerf import mesh_export
    sig = inspect.signature(type(host_model).extract_mesh).parameters
    defaults = {k: p.default for k, p in sig.items() if k != 'self'}
    o = mesh_export.parse_options(host_model, **{**defaults, 'resolution': 8, 'tsdf': TSDF, 'color_views': 'tsdf', 'color': True, 'remesh': 12})
    assert o.R == 8 and o.tsdf_cfg['trunc'] == 4.0 * float(o.step.max()) and o.cv_cfg['depth_tol'] == 2.0 * float(o.step.max())
    assert o.remesh_kw == {'resolution': 12} and o.cv_cfg['min_opacity'] == 0.9 and 'trunc' not in o.cv_cfg
    with pytest.raises(Exception) as e:
        host_model.extract_mesh(resolution=8)
    assert not isinstance(e.value, ValueError)
