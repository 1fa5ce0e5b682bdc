"""Mesh export of a trained field, in stages: what NeRFRenderer.extract_mesh / save_mesh / render_depth / render_view run.  The API and its
documentation are those methods' signatures and docstrings (nerf/renderer.py); the kernels are mesh.py's.  Plain functions that take the
model first and reach the field only through it (model.density_volume, model._mesh_sigma, model.render_depth, model.render_view,
model(x, d)), so that an instance that replaces one of those is honoured.

    parse_options   every check, to completion, before the first launch or render -> Options
    surface_*       tsdf | sparse | dense           -> (verts, faces, normals, vol, threshold, info)
    repair          component removal, fill_holes   -> the surface 'deviation' and bake_from='source' compare with
    lossy           remesh, smooth, simplify, decimate
    colour          color_fn (field query, or ViewColors over the surface the queried points lie on), vertex colours, bake_texture
    reports         the result dict: topology, deviation, ao
"""
import math
from collections import namedtuple

import numpy as np
import torch

from .. import raymarching, mesh as _mesh


# ------------------------------------------------------------------------------------------------ options
_CAMERA_KEYS = {'poses': None, 'intrinsics': None, 'H': None, 'W': None, 'convention': 'nerfstudio', 'min_opacity': 0.5, 'render': None}
TSDF_KEYS = {**_CAMERA_KEYS, 'trunc': None, 'carve': True}
COLOR_VIEW_KEYS = {**_CAMERA_KEYS, 'depth_tol': None, 'power': 2, 'min_cos': 0.2}


def camera_set(opt, name, keys, min_size, finite):
    """The camera set of extract_mesh's `name`= dict (tsdf or color_views), with the defaults of `keys` filled in: poses [N, 3|4, 4] as a
    host float32 tensor (finite, if `finite`), intrinsics as 4 floats, H, W >= min_size, convention, min_opacity, render -> the dict"""
    unknown = sorted(set(opt) - set(keys))
    if unknown:
        raise ValueError(f"extract_mesh: unknown {name} keys {unknown}; known: {sorted(keys)}")
    missing = [k for k in ('poses', 'intrinsics', 'H', 'W') if opt.get(k) is None]
    if missing:
        raise ValueError(f"extract_mesh: {name} needs {missing}")
    cfg = {**keys, **opt}
    p = cfg['poses']
    p = torch.as_tensor(np.asarray(p.detach().cpu() if torch.is_tensor(p) else p, dtype=np.float32))
    if p.dim() != 3 or tuple(p.shape[1:]) not in ((3, 4), (4, 4)):
        raise ValueError(f"extract_mesh: {name}['poses'] must be [N, 3, 4] or [N, 4, 4], got {tuple(p.shape)}")
    if p.shape[0] == 0:
        raise ValueError(f"extract_mesh: {name}['poses'] holds no view")
    if finite and not bool(torch.isfinite(p).all()):
        raise ValueError(f"extract_mesh: {name}['poses'] holds non-finite values")
    if cfg['convention'] not in ('nerfstudio', 'ngp'):
        raise ValueError(f"extract_mesh: {name}['convention'] must be 'nerfstudio' or 'ngp', got {cfg['convention']!r}")
    k = tuple(float(x) for x in cfg['intrinsics'])
    if len(k) != 4:
        raise ValueError(f"extract_mesh: {name}['intrinsics'] must be (fx, fy, cx, cy), got {len(k)} values")
    H, W = int(cfg['H']), int(cfg['W'])
    if H < min_size or W < min_size:
        raise ValueError(f"extract_mesh: {name} needs H, W >= {min_size}, got {H}, {W}")
    cfg.update(poses=p, intrinsics=k, H=H, W=W, min_opacity=float(cfg['min_opacity']), render=dict(cfg['render'] or {}))
    return cfg


def tsdf_options(tsdf, sparse, part, max_step):
    """extract_mesh's tsdf= dict with its defaults filled in; everything wrong with it raises ValueError before any render"""
    if not isinstance(tsdf, dict):
        raise ValueError(f"extract_mesh: tsdf must be None or a dict of options, got {type(tsdf).__name__}")
    if sparse:
        raise ValueError("extract_mesh: tsdf and sparse=True exclude each other (a brick-sparse TSDF is not built)")
    if part != 'all':
        raise ValueError(f"extract_mesh: tsdf fuses renders of the whole field; part must be 'all', got {part!r}")
    cfg = camera_set(tsdf, 'tsdf', TSDF_KEYS, 1, finite=False)
    trunc = 4.0 * max_step if cfg['trunc'] is None else float(cfg['trunc'])
    if not (math.isfinite(trunc) and trunc > 0.0):
        raise ValueError(f"extract_mesh: tsdf['trunc'] must be finite and > 0, got {cfg['trunc']}")
    cfg.update(trunc=trunc, carve=bool(cfg['carve']))
    return cfg


def color_view_options(color_views, tsdf, wanted, max_step):
    """extract_mesh's color_views= (a dict, or 'tsdf' for the cameras of `tsdf`) with its defaults filled in; everything wrong with it
    raises ValueError before any render.  `wanted`: color=True or texture=R was asked for."""
    if isinstance(color_views, str):
        if color_views != 'tsdf':
            raise ValueError(f"extract_mesh: color_views must be None, a dict of options or 'tsdf', got {color_views!r}")
        if not isinstance(tsdf, dict):
            raise ValueError("extract_mesh: color_views='tsdf' reuses the cameras of tsdf=, which is not given")
        color_views = {k: tsdf[k] for k in _CAMERA_KEYS if k in tsdf}
    if not isinstance(color_views, dict):
        raise ValueError(f"extract_mesh: color_views must be None, a dict of options or 'tsdf', got {type(color_views).__name__}")
    if not wanted:
        raise ValueError("extract_mesh: color_views colours the vertices or a texture; it needs color=True or texture=R")
    cfg = camera_set(color_views, 'color_views', COLOR_VIEW_KEYS, 2, finite=True)
    tol = 2.0 * max_step if cfg['depth_tol'] is None else float(cfg['depth_tol'])
    if not (math.isfinite(tol) and tol > 0.0):
        raise ValueError(f"extract_mesh: color_views['depth_tol'] must be finite and > 0, got {cfg['depth_tol']}")
    power, min_cos = cfg['power'], float(cfg['min_cos'])
    if isinstance(power, bool) or not isinstance(power, (int, np.integer)) or not 1 <= power <= 8:
        raise ValueError(f"extract_mesh: color_views['power'] must be an integer in 1..8, got {power!r}")
    if not 0.0 <= min_cos < 1.0:
        raise ValueError(f"extract_mesh: color_views['min_cos'] must lie in [0, 1), got {cfg['min_cos']}")
    cfg.update(depth_tol=tol, power=int(power), min_cos=min_cos)
    return cfg


# extract_mesh's arguments, checked and normalised by parse_options: all a stage may read besides the mesh it is handed, and read-only.
# R, lo, step: the lattice (points per axis; lower corner and step, [3] host tensors); fill / fill_edges: fill_holes and its longest loop;
# k: simplify's cluster size; tf: target_faces; reach: bake_reach or its default; tsdf_cfg / cv_cfg: None or the options' dicts
Options = namedtuple('Options', 'R lo step threshold aabb chunk part view_dir color min_component_faces keep_largest fill fill_edges remesh_kw '
                                'n_smooth smooth_lambda smooth_mu k tf tex_r texture_layout normal_map from_source reach sparse sparse_probe '
                                'tsdf_cfg cv_cfg deviation deviation_spacing deviation_max_samples n_ao topology field_normals')


def parse_options(model, *, resolution, threshold, aabb, chunk, part, view_dir, color, min_component_faces, keep_largest, simplify,
                  target_faces, texture, smooth, smooth_lambda, smooth_mu, deviation, deviation_spacing, deviation_max_samples, ao,
                  texture_layout, bake_from, bake_reach, normal_map, sparse, sparse_probe, tsdf, fill_holes, topology, color_views, remesh,
                  normals='mesh'):
    """Every check extract_mesh makes on its arguments (NeRFRenderer.extract_mesh gives their defaults and meaning), none of which
    touches the device -> Options"""
    if fill_holes is True or fill_holes is False:
        fill_edges = None
    elif isinstance(fill_holes, (int, np.integer)) and fill_holes >= 3:
        fill_edges = int(fill_holes)
    else:
        raise ValueError(f"extract_mesh: fill_holes must be False, True (no length limit) or an int >= 3 (the longest loop filled), "
                         f"got {fill_holes!r}")
    if normals not in ('mesh', 'field'):
        raise ValueError(f"extract_mesh: normals must be 'mesh' or 'field', got {normals!r}")
    if normals == 'field' and (part != 'all' or tsdf is not None or remesh is not None):
        raise ValueError("extract_mesh: normals='field' are the normals of the density's level set; the surfaces of part='fg' / 'bg', tsdf= and "
                         "remesh= are not one")
    if fill_holes is not False and int(simplify):
        raise ValueError("extract_mesh: fill_holes and simplify exclude each other (clustered meshes need not be manifold)")
    threshold = float(model.opt.density_thresh if threshold is None else threshold)
    R = int(resolution)
    lo, step = model._mesh_lattice(R, aabb)
    k = int(simplify)
    if k == 1 or k < 0:
        raise ValueError(f"extract_mesh: simplify must be 0 (off) or a cluster size >= 2 lattice steps, got {simplify}")
    tf = int(target_faces)
    if tf < 0:
        raise ValueError(f"extract_mesh: target_faces must be 0 (off) or a face count, got {target_faces}")
    if tf and k:
        raise ValueError("extract_mesh: target_faces and simplify exclude each other (clustered meshes need not be manifold)")
    tex_r = int(texture)
    if tex_r < 0:
        raise ValueError(f"extract_mesh: texture must be 0 (off) or a texture resolution, got {texture}")
    if texture_layout not in _mesh.TEXTURE_LAYOUTS:
        raise ValueError(f"extract_mesh: texture_layout must be 'uniform', 'area' or 'projected', got {texture_layout!r}")
    n_smooth = int(smooth)
    if n_smooth < 0:
        raise ValueError(f"extract_mesh: smooth must be 0 (off) or a number of iterations, got {smooth}")
    n_ao = int(ao)
    if n_ao < 0:
        raise ValueError(f"extract_mesh: ao must be 0 (off) or a number of rays per vertex, got {ao}")
    if bake_from not in ('mesh', 'source'):
        raise ValueError(f"extract_mesh: bake_from must be 'mesh' or 'source', got {bake_from!r}")
    from_source = bake_from == 'source'
    if isinstance(normal_map, str) and normal_map != 'tangent':
        raise ValueError(f"extract_mesh: normal_map must be False, True (object space) or 'tangent', got {normal_map!r}")
    if normal_map and not tex_r:
        raise ValueError(f"extract_mesh: normal_map={normal_map!r} needs texture=R, the resolution of the atlas it shares")
    max_step = float(step.max())
    reach = 4.0 * max_step if bake_reach is None else float(bake_reach)
    if from_source and not reach > 0.0:
        raise ValueError(f"extract_mesh: bake_reach must be > 0, got {bake_reach}")
    if int(sparse_probe) < 1:
        raise ValueError(f"extract_mesh: sparse_probe must be >= 1 (every how many lattice points the field is probed), got {sparse_probe}")
    remesh_kw = None
    if remesh is not None:
        if isinstance(remesh, dict):
            remesh_kw = dict(remesh)
        elif isinstance(remesh, (int, np.integer)) and not isinstance(remesh, bool):
            remesh_kw = {'resolution': int(remesh)}
        else:
            raise ValueError(f"extract_mesh: remesh must be None, a resolution (int) or a dict of mesh.voxel_remesh's options, got {remesh!r}")
        unknown = set(remesh_kw) - {'resolution', 'voxel', 'offset', 'beta', 'probe'}
        if unknown or (remesh_kw.get('resolution') is None) == (remesh_kw.get('voxel') is None):
            raise ValueError(f"extract_mesh: remesh takes exactly one of 'resolution' and 'voxel', and 'offset', 'beta', 'probe'; "
                             f"got {sorted(remesh_kw)}")
    cv_cfg = None if color_views is None else color_view_options(color_views, tsdf, bool(color) or bool(tex_r), max_step)
    tsdf_cfg = None if tsdf is None else tsdf_options(tsdf, sparse, part, max_step)
    return Options(R=R, lo=lo, step=step, threshold=threshold, aabb=aabb, chunk=chunk, part=part, view_dir=view_dir, color=color,
                   min_component_faces=int(min_component_faces), keep_largest=bool(keep_largest), fill=fill_holes is not False,
                   fill_edges=fill_edges, remesh_kw=remesh_kw, n_smooth=n_smooth, smooth_lambda=smooth_lambda, smooth_mu=smooth_mu, k=k,
                   tf=tf, tex_r=tex_r, texture_layout=texture_layout, normal_map=normal_map, from_source=from_source, reach=reach,
                   sparse=sparse, sparse_probe=int(sparse_probe), tsdf_cfg=tsdf_cfg, cv_cfg=cv_cfg, deviation=deviation,
                   deviation_spacing=deviation_spacing, deviation_max_samples=deviation_max_samples, n_ao=n_ao, topology=topology, field_normals=normals == 'field')


# ------------------------------------------------------------------------------------------------ the surface
def surface_tsdf(model, o):
    """render_depth from every pose, fused into a TSDF on the lattice, and its zero level"""
    cfg = o.tsdf_cfg
    poses = cfg['poses']
    tv = _mesh.TSDFVolume((o.R,) * 3, o.lo.tolist(), o.step.tolist(), cfg['trunc'], device=model.aabb_infer.device)
    for s in range(0, poses.shape[0], 16):                                       # a launch of the fusion takes 16 views: the volume is read once for them
        maps = []
        for pose in poses[s:s + 16]:
            d = model.render_depth(pose, cfg['intrinsics'], cfg['H'], cfg['W'], convention=cfg['convention'],
                                   min_opacity=cfg['min_opacity'], **cfg['render'])['depth']
            maps.append(d if cfg['carve'] else torch.where(torch.isinf(d), torch.full_like(d, math.nan), d))
        tv.integrate(torch.stack(maps), poses[s:s + 16], cfg['intrinsics'], convention=cfg['convention'], depth_kind='ray')
    vol = tv.volume()
    verts, faces, normals, info = tv.extract()
    return verts, faces, normals, vol, 0.0, {'tsdf': {'views': tv.views, 'trunc': tv.trunc, 'observed': info['observed'],
                                                      'dropped_faces': info['dropped_faces']}}


def surface_sparse(model, o):
    """the field probed coarsely, then evaluated only in the bricks round the surface, and marching cubes over the brick list"""
    sv = _mesh.sparse_volume(lambda x: model._mesh_sigma(x, o.part, o.view_dir), (o.R,) * 3, o.lo, o.step, o.threshold, probe=o.sparse_probe,
                             chunk=o.chunk, device=model.aabb_infer.device)
    verts, faces, normals = _mesh.marching_cubes_sparse(sv, o.threshold)
    return verts, faces, normals, None, o.threshold, {'sparse': {'bricks': sv.n_bricks, 'evaluations': sv.evaluations, 'rounds': sv.rounds,
                                                                 'points': o.R ** 3}}


def surface_dense(model, o):
    """density_volume, then marching cubes"""
    vol = model.density_volume(o.R, o.aabb, o.chunk, o.part, o.view_dir)
    verts, faces, normals = _mesh.marching_cubes(vol, o.threshold, spacing=o.step.tolist(), origin=o.lo.tolist())
    return verts, faces, normals, vol, o.threshold, {}


# ------------------------------------------------------------------------------------------------ repair, then the lossy passes
def repair(o, verts, faces, normals):
    """component removal, then fill_holes -> (verts, faces, normals, info)"""
    info = {}
    if o.min_component_faces > 0 or o.keep_largest:
        verts, faces, normals, _ = _mesh.remove_small_components(verts, faces, normals, min_faces=o.min_component_faces, largest=o.keep_largest)
    if o.fill:
        verts, faces, normals, info['holes'] = _mesh.fill_holes(verts, faces, normals, max_edges=o.fill_edges)
    return verts, faces, normals, info


def lossy(o, verts, faces, normals):
    """remesh, smooth, simplify, decimate -> (verts, faces, normals, info, whether any of them ran)"""
    info = {}
    if o.remesh_kw is not None:
        verts, faces, normals, info['remesh'] = _mesh.voxel_remesh(verts, faces, chunk=o.chunk, **o.remesh_kw)
    if o.n_smooth:
        verts, normals = _mesh.smooth(verts, faces, o.n_smooth, o.smooth_lambda, o.smooth_mu, normals=normals)
    if o.k >= 2:
        g = (-(-(o.R - 1) // o.k),) * 3                                          # ceil((R - 1) / k) cells cover the lattice
        verts, faces, normals = _mesh.simplify(verts, faces, (o.step * o.k).tolist(), normals=normals, origin=o.lo.tolist(), grid=g)
    if o.tf:
        verts, faces, normals, _ = _mesh.decimate(verts, faces, o.tf, normals=normals)
    return verts, faces, normals, info, bool(o.remesh_kw is not None or o.n_smooth or o.k >= 2 or o.tf)


def field_normals(model, o, verts, normals):
    """the field's own normals at the vertices (model.normal); a vertex keeps its geometric normal where the field's is zero or opposes it
    -> (normals, {'kept_geometric': how many kept theirs})"""
    out = torch.empty_like(normals)
    kept = torch.zeros((), dtype=torch.int64, device=verts.device)
    for s in range(0, verts.shape[0], o.chunk):
        geo = normals[s:s + o.chunk]
        n = model.normal(verts[s:s + o.chunk].contiguous())
        keep = (n * geo).sum(-1) <= 0
        out[s:s + o.chunk] = torch.where(keep[:, None], geo, n)
        kept += keep.sum()
    return out, {'kept_geometric': int(kept)}


# ------------------------------------------------------------------------------------------------ colour
def view_colors(model, cfg, verts, faces, fallback):
    """mesh.ViewColors of the views of cfg (color_view_options) on the surface (verts, faces): every pose rendered with render_view —
    its opacity is the pixel weight, zero below min_opacity — and the surface rasterised from it for the visibility depth"""
    images, depths, weights = [], [], []
    for pose in cfg['poses']:
        rv = model.render_view(pose, cfg['intrinsics'], cfg['H'], cfg['W'], convention=cfg['convention'], min_opacity=cfg['min_opacity'],
                               **cfg['render'])
        images.append(rv['image'])
        weights.append(torch.where(rv['opacity'] >= cfg['min_opacity'], rv['opacity'], torch.zeros_like(rv['opacity'])))
        depths.append(_mesh.rasterize(verts, faces, pose, cfg['intrinsics'], cfg['H'], cfg['W'], convention=cfg['convention'])['depth'])
    return _mesh.ViewColors(torch.stack(images), torch.stack(depths), cfg['poses'], cfg['intrinsics'], cfg['depth_tol'],
                            convention=cfg['convention'], depth_kind='z', weights=torch.stack(weights), power=cfg['power'],
                            min_cos=cfg['min_cos'], fallback=fallback)


def colour(model, o, verts, faces, normals, kept):
    """Vertex colours and the baked texture of the final mesh (verts, faces, normals); `kept` is the surface as it stood after repair, which
    bake_from='source' projects onto.  -> (colors or None, uvs, texture, extra: the keys colour adds to the result)"""
    source = _mesh.bake_source(*kept) if o.from_source and (o.color or o.tex_r) else None
    kinds = torch.zeros(4, dtype=torch.int64, device=verts.device) if o.from_source else None
    field_color = lambda x, d: model(x, d)[1][:, :3]                            # noqa: E731
    color_fn = field_color
    if o.cv_cfg is not None:                                                     # the views on the surface the queried points lie on
        color_fn = view_colors(model, o.cv_cfg, *(kept[:2] if source is not None else (verts, faces)), field_color)
    colors = None
    if o.color:
        colors = torch.empty(verts.shape[0], 3, dtype=torch.uint8, device=verts.device)
        for s in range(0, verts.shape[0], o.chunk):
            x, look = verts[s:s + o.chunk].contiguous(), (-normals[s:s + o.chunk]).contiguous()
            if source is not None:
                pr = _mesh.project_to_surface(source, x, normals[s:s + o.chunk], o.reach)
                x, look = pr['point'], -pr['normal']
                if not o.tex_r:
                    kinds += (pr['kind'][:, None] == torch.arange(4, dtype=torch.uint8, device=x.device)).sum(0)
            rgb = color_fn(x, look).float()
            colors[s:s + o.chunk] = (rgb.clamp(0, 1) * 255).round().to(torch.uint8)
    uvs = tex = nmap = tangents = None
    if o.tex_r:
        baked = _mesh.bake_texture(verts, faces, o.tex_r, color_fn, normals=normals, chunk=o.chunk, layout=o.texture_layout, source=source,
                                   reach=o.reach if source is not None else None,
                                   normal_map=o.normal_map if isinstance(o.normal_map, str) else bool(o.normal_map))
        uvs, tex = baked[:2]
        if len(baked) > 2:
            nmap, kinds = baked[2]['normal_map'], baked[2]['kinds'] if source is not None else kinds
            tangents = baked[2].get('tangents')
    extra = {}
    if o.cv_cfg is not None:
        extra['view_colors'] = {'views': color_fn.views, 'seen': color_fn.counts, 'depth_tol': color_fn.depth_tol}
    if o.normal_map:
        extra['normal_map'] = nmap
        extra['normal_space'] = 'tangent' if isinstance(o.normal_map, str) else 'object'
    if isinstance(o.normal_map, str):
        extra['tangents'] = tangents
    if o.from_source:
        extra['bake_kinds'] = kinds
    return colors, uvs, tex, extra


# ------------------------------------------------------------------------------------------------ the pipeline
def extract_mesh(model, **kw):
    """NeRFRenderer.extract_mesh: the stages, each handed the mesh of the one before"""
    o = parse_options(model, **kw)
    surface = surface_tsdf if o.tsdf_cfg is not None else surface_sparse if o.sparse else surface_dense
    verts, faces, normals, vol, threshold, surface_info = surface(model, o)
    verts, faces, normals, repair_info = repair(o, verts, faces, normals)
    kept = (verts, faces, normals) if o.deviation or o.from_source else None    # held only for the report and the projection
    verts, faces, normals, lossy_info, changed = lossy(o, verts, faces, normals)
    if o.field_normals:
        normals, lossy_info['field_normals'] = field_normals(model, o, verts, normals)
    colors, uvs, tex, colour_info = colour(model, o, verts, faces, normals, kept)
    return {'verts': verts, 'faces': faces, 'normals': normals, 'colors': colors, 'volume': vol, 'threshold': threshold,
            'uvs': uvs, 'texture': tex, 'texture_layout': o.texture_layout, **surface_info, **repair_info, **lossy_info, **colour_info,
            **reports(o, verts, faces, normals, kept, changed)}


def reports(o, verts, faces, normals, kept, changed):
    """What was asked about the final mesh: topology, its deviation from `kept` (None unless a lossy pass `changed` it), ambient occlusion"""
    m = {}
    if o.topology:
        m['topology'] = _mesh.topology(verts, faces)
    if o.deviation:
        m['deviation'] = None
        if changed:
            sp = 0.5 * float(o.step.min()) if o.deviation_spacing is None else float(o.deviation_spacing)
            m['deviation'] = dict(_mesh.distance(verts, faces, kept[0], kept[1], spacing=sp, max_samples=o.deviation_max_samples),
                                  step=tuple(o.step.tolist()))
    if o.n_ao:
        m['ao'] = _mesh.ambient_occlusion(verts, faces, normals=normals, samples=o.n_ao)
    return m


def save_mesh(model, path, **kw):
    """NeRFRenderer.save_mesh: what the format cannot carry is refused before the extraction"""
    obj, glb = (str(path).lower().endswith(e) for e in (".obj", ".glb"))
    nm = kw.get('normal_map')
    if int(kw.get('texture', 0) or 0) and not (obj or glb):
        raise ValueError(f"save_mesh: texture= needs an .obj or .glb path (PLY carries no texture), got {path!r}")
    if nm and not (obj or glb):
        raise ValueError(f"save_mesh: normal_map={nm!r} needs an .obj or .glb path (PLY carries no normal map), got {path!r}")
    if glb and nm and nm != 'tangent':
        raise ValueError("save_mesh: glTF has no slot for an object-space normal map; use normal_map='tangent' with a .glb path")
    if obj and nm == 'tangent':
        raise ValueError("save_mesh: OBJ carries no tangents; normal_map='tangent' needs a .glb path")
    normals = kw.pop('normals', 'mesh')
    m = model.extract_mesh(**kw) if normals == 'mesh' else model.extract_mesh_normals(normals, **kw)
    if obj:
        _mesh.write_obj(path, m['verts'], m['faces'], uvs=m['uvs'], normals=m['normals'], texture=m['texture'], normal_map=m.get('normal_map'))
    elif glb and m['uvs'] is not None:
        g = _mesh.gltf_vertices(m['verts'], m['faces'], m['uvs'], m['normals'])
        _mesh.write_glb(path, g['positions'], g['indices'], normals=g['normals'], uvs=g['uvs'], tangents=g['tangents'],
                        texture=m['texture'], normal_map=m.get('normal_map'))
    else:                                                                        # vertex colours; without them the ambient occlusion as grey
        colors = m['colors']
        if colors is None and 'ao' in m:
            colors = (m['ao'] * 255).round().to(torch.uint8)[:, None].expand(-1, 3)
        write = _mesh.write_glb if glb else _mesh.write_ply
        write(path, m['verts'], m['faces'], normals=m['normals'], colors=colors)
    return m


# ------------------------------------------------------------------------------------------------ rendered views
SHADINGS = ('normal', 'lambertian', 'textureless')
VIEW_OPTIONS = {'normals': False, 'shading': None, 'light_d': None, 'ambient_ratio': 0.1, 'path': None}     # render_view's own keywords


def render_view(model, c2w, intrinsics, H, W, convention, min_opacity, max_ray_batch, render_kw, want_image, what, normals=False, shading=None,
                light_d=None, ambient_ratio=0.1, path=None):
    """NeRFRenderer.render_view (want_image) and render_depth (not): one pass of model.render per ray batch -> {'image' if wanted, 'depth',
    'opacity'}; `what` names the caller in the messages.  normals / shading / light_d / ambient_ratio / path: render_view's docstring."""
    if shading is not None and shading not in SHADINGS:
        raise ValueError(f"{what}: shading must be None or one of {SHADINGS}, got {shading!r}")
    if not 0.0 <= float(ambient_ratio) <= 1.0:
        raise ValueError(f"{what}: ambient_ratio must lie in [0, 1], got {ambient_ratio}")
    normals = bool(normals) or shading is not None
    if normals:
        render_kw = dict(render_kw, normals=True)
    m = torch.as_tensor(np.asarray(c2w.detach().cpu() if torch.is_tensor(c2w) else c2w, dtype=np.float32))
    if tuple(m.shape) not in ((3, 4), (4, 4)):
        raise ValueError(f"{what}: c2w must be [3, 4] or [4, 4], got {tuple(m.shape)}")
    k = tuple(float(x) for x in intrinsics)
    H, W, batch = int(H), int(W), int(max_ray_batch)
    if len(k) != 4 or H < 1 or W < 1 or batch < 1:
        raise ValueError(f"{what}: need intrinsics (fx, fy, cx, cy), H, W >= 1 and max_ray_batch >= 1, got {k}, {H}, {W}, {batch}")
    from .provider_utils import generate_rays
    dev = model.aabb_infer.device
    o, d = generate_rays(m[None, :3].to(dev), *k, H, W, 1.0, convention)
    o, d = o.view(-1, 3), d.view(-1, 3)
    image = torch.empty(H * W, 3, dtype=torch.float32, device=dev) if want_image else None
    depth = torch.empty(H * W, dtype=torch.float32, device=dev)
    opacity = torch.empty_like(depth)
    nmap = torch.empty(H * W, 3, dtype=torch.float32, device=dev) if normals else None
    aabb = model.aabb_train if model.training else model.aabb_infer
    for s in range(0, H * W, batch):
        ro, rd = o[s:s + batch].contiguous(), d[s:s + batch].contiguous()
        res = model.render(ro[None], rd[None], staged=True, perturb=False, **render_kw)
        if 'depth' not in res or (want_image and 'image' not in res):
            raise ValueError(f"{what}: render() returned no {'image or ' if want_image else ''}depth (run() fills its results only under "
                             f"opt.train_conf)")
        acc = res['weights_sum'].reshape(-1).float()
        t = res['depth'].reshape(-1).float() / acc                              # 0 / 0 where nothing was hit: below min_opacity anyway
        if not model.cuda_ray:
            near, far = raymarching.near_far_from_aabb(ro, rd, aabb, model.min_near)
            t = near + t * (far - near)
        depth[s:s + batch] = t * rd.norm(dim=-1)
        opacity[s:s + batch] = acc
        if want_image:
            image[s:s + batch] = res['image'].reshape(-1, 3).float()
        if normals:
            nmap[s:s + batch] = res['normal_map'].reshape(-1, 3)
    hit = opacity >= float(min_opacity)
    depth = torch.where(hit, depth, torch.full_like(depth, math.inf))
    out = {'depth': depth.view(H, W), 'opacity': opacity.view(H, W)}
    if want_image:
        out = {'image': image.view(H, W, 3), **out}
    if normals:
        # the composited sum w n is shorter than 1 by the spread of the samples' normals: renormalised per pixel (zero stays zero)
        length = nmap.norm(dim=-1, keepdim=True)
        n = torch.where(hit[:, None] & (length > 0), nmap / length.clamp_min(1e-20), torch.zeros_like(nmap))
        out['normal'] = n.view(H, W, 3)
        if shading == 'normal':
            out['shaded'] = ((n + 1) / 2).view(H, W, 3)
        elif shading is not None:
            # deferred shading of the composited normal (one evaluation per pixel, not per sample)
            # default light: at the camera, i.e. against the view direction (the ray of the centre pixel)
            light = -d[(H // 2) * W + W // 2] if light_d is None else torch.as_tensor(light_d, dtype=torch.float32, device=dev)
            light = light.reshape(3) / light.norm().clamp_min(1e-20)
            lam = float(ambient_ratio) + (1 - float(ambient_ratio)) * (n @ light).clamp_min(0)[:, None]
            out['shaded'] = ((image if shading == 'lambertian' else 1.0) * lam).expand(H * W, 3).reshape(H, W, 3)
    if path is not None:
        pic = out.get('shaded', (out['normal'] + 1) / 2 if normals else out.get('image', None))
        if pic is None:
            raise ValueError(f"{what}: path= needs an image to write")
        _mesh.write_png(path, (pic.clamp(0, 1) * 255).round().to(torch.uint8))
    return out
