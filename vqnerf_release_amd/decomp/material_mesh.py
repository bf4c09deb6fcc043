"""The exported mesh, cut into its materials: the VQ code of every vertex of a mesh (geo `Runner.validate_mesh` writes one; its vertices
are in the frame of the decomposition's `xyz`), cleaned up over the mesh, one code per face, and the mesh split into one sub-mesh per
code -- in files another tool opens.  The networks run at the vertices through `Model.materials_at`; the mesh side is
csrc/mesh_materials.hip through geo/mesh.py (`smooth_labels`, `split_by_label`).  DESIGN.md section 16.

  run   outdir/material_mesh.ply    the whole mesh; per vertex red green blue (the diffuse colour (1 - ks) basecolor, linear -> sRGB,
                                    8 bit), float spec, float rough, int material (the smoothed code)
        outdir/material_mesh.obj    the faces sorted by code, one `usemtl code_%03d` per used code
        outdir/material_mesh.mtl    per code Kd (1 - ks) basecolor, Ks ks basecolor, Pr rough, Ns, illum 2
        outdir/code_%03d.ply        with parts=True: one sub-mesh per used code (or per code of `codes`), its own compact vertex list
        outdir/material_mesh.json   K; per code vertices, faces, surface area, connected regions; changed per smoothing round; dropped faces
        outdir/material_mesh_view_%03d_{albedo,material,rough}.png
                                    with views=[(P, H, W), ...]: the mesh drawn from each camera (geo/mesh_render.py): the diffuse colour
                                    (linear -> sRGB over white), the code of the nearest corner through segmentation.PD_PALETTE (black off
                                    the mesh: the image segmentation.scores takes against a hand-labelled idx.png), the roughness

The driver takes the model, as decomp/materials.py does (a stage-3 model stands for the stage-2 model it was loaded from)."""
import json
import os

import torch

from vqnerf_release_amd import _C
from vqnerf_release_amd.decomp.nerfactor.util import img as imgutil
from vqnerf_release_amd.geo import mesh as meshutil

NS_MAX = 1000.0               # the largest specular exponent an MTL holds


def _u8(linear):
    """the project's 8-bit sRGB bytes of linear colours (util/img.py, as vis.to_uint8 quantises them)"""
    return (torch.clamp(imgutil.linear2srgb(linear.float().contiguous()), 0.0, 1.0) * 255.0).to(torch.uint8)


def mtl_rows(rows):
    """material rows float32 [K, 7] = albedo[3], f0[3], rough[1] (Model.material_rows: albedo = (1 - ks) basecolor, f0 = ks basecolor,
    as init_mat composes them) -> one dict per code for mesh.write_mtl.  Ns = clip(2 / alpha^2 - 2, 0, 1000), the Blinn-Phong exponent
    of a GGX lobe of width alpha, with alpha = rough^2 -- the `alpha` of util/microfacet.py, before that file squares it once more
    inside D and G."""
    r = rows.detach().double().cpu()
    alpha = r[:, 6] ** 2
    ns = torch.clamp(2.0 / torch.clamp(alpha ** 2, min=1e-300) - 2.0, 0.0, NS_MAX)
    return [dict(Kd=r[k, 0:3].tolist(), Ks=r[k, 3:6].tolist(), Pr=float(r[k, 6]), Ns=float(ns[k]), illum=2) for k in range(r.shape[0])]


def face_areas(vertices, triangles):
    """float64 [T] (device): half the length of the cross product of two edges, formed in float64 from the f32 vertices"""
    p = vertices.double()[triangles.long()]
    return 0.5 * torch.linalg.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]).norm(dim=-1)


def region_counts(triangles, codes, n_codes):
    """int64 [K] (device): per code the connected regions of the mesh that carry it -- the components of the graph whose nodes are the
    vertices a triangle uses and whose edges are the triangle edges with the same code at both ends.  Through vqn_mesh_components,
    given one degenerate triangle (a, b, b) per such edge ((a, a, a), which connects nothing, for the others)."""
    V = codes.shape[0]
    t = triangles.long()
    a = torch.cat([t[:, 0], t[:, 1], t[:, 2]])
    b = torch.cat([t[:, 1], t[:, 2], t[:, 0]])
    ok = (a >= 0) & (a < V) & (b >= 0) & (b < V)
    a, b = torch.where(ok, a, torch.zeros_like(a)), torch.where(ok, b, torch.zeros_like(b))
    same = ok & (codes[a] == codes[b])
    b = torch.where(same, b, a)
    edges = torch.stack([a, b, b], -1).to(torch.int32).contiguous()
    labels = _C.mesh_components(edges, V).long()
    used = torch.zeros((V,), dtype=torch.int32, device=codes.device).scatter_add_(0, a, ok.to(torch.int32)) > 0     # (integer adds: exact)
    roots = used & (labels == torch.arange(V, device=codes.device))
    c = codes.long()
    roots &= (c >= 0) & (c < n_codes)
    return torch.zeros((n_codes,), dtype=torch.int64, device=codes.device).scatter_add_(0, c.clamp(0, n_codes - 1), roots.long())


def write_views(outdir, vertices, triangles, views, diffuse, label, rough):
    """material_mesh_view_%03d_{albedo,material,rough}.png per camera (P, H, W) of `views` -> one row per view for the record"""
    from PIL import Image
    from vqnerf_release_amd.geo import mesh_render
    rows = []
    for i, (P, H, W) in enumerate(views):
        r = mesh_render.render(vertices, triangles, P, int(H), int(W), colors=diffuse.float(), labels=label, background=1.0)
        rough_img = mesh_render.interpolate(r, triangles, rough.float(), background=0.0)
        albedo = torch.where(r['mask'][..., None], _u8(r['color'].reshape(-1, 3)).reshape(int(H), int(W), 3), torch.full_like(r['label'], 255))
        images = {'albedo': albedo, 'material': r['label'],
                  'rough': (torch.clamp(rough_img, 0.0, 1.0) * 255.0).to(torch.uint8)}
        for name, img in images.items():
            Image.fromarray(img.cpu().numpy()).save(os.path.join(outdir, 'material_mesh_view_%03d_%s.png' % (i, name)))
        rows.append({'view': i, 'H': int(H), 'W': int(W), 'pixels': int(r['mask'].sum()), 'stats': r['stats']})
    return rows


@torch.no_grad()
def run(model, mesh, outdir, smooth=2, self_weight=1, branch='vq', parts=False, codes=None, log=None, views=None):
    """-> the record written to outdir/material_mesh.json.  mesh: the path of a PLY file (mesh.read_ply) or (vertices [V, 3] f32,
    triangles [T, 3] int32[, normals [V, 3]]) on the device.  smooth / self_weight: the rounds and the own-code weight of
    mesh.smooth_labels.  branch: 'vq' -- every vertex shows material_rows()[its smoothed code], piecewise constant and equal to the
    MTL -- or 'main', the continuous heads at the vertex.  parts: also one code_%03d.ply per used code, or per code of `codes`.
    views: a list of cameras (P [3, 4] on the host, H, W) as mesh_render.camera_from_rays gives them: three images per view of the
    per-vertex values above; None writes nothing more and leaves the record as it is."""
    if branch not in ('vq', 'main'):
        raise ValueError(f"branch is 'vq' or 'main', got {branch!r}")
    if isinstance(mesh, (str, os.PathLike)):
        mesh = meshutil.read_ply(mesh)
    vertices, triangles = mesh[0], mesh[1]
    normals = mesh[2] if len(mesh) > 2 else None
    if triangles is None:
        raise _C.VqnError('material_mesh.run: the mesh has no faces')
    vertices, triangles = vertices.detach().float().contiguous(), triangles.detach().to(torch.int32).contiguous()
    rows = model.material_rows()
    K = rows.shape[0]
    at = model.materials_at(vertices)
    label, changed = meshutil.smooth_labels(triangles, at['code'], K, iters=smooth, self_weight=self_weight)
    split = meshutil.split_by_label(triangles, label, K)
    # (the one float `spec` of a vertex is the largest channel of its specular colour f0: exact, and f0 itself when the channels agree)
    if branch == 'vq':
        picked = rows[label.long()]
        diffuse, spec, rough = picked[:, 0:3], picked[:, 3:6].max(-1)[0], picked[:, 6]
    else:
        diffuse, spec, rough = (1 - at['ks']) * at['basecolor'], (at['ks'] * at['basecolor']).max(-1)[0], at['rough'][:, 0]
    os.makedirs(outdir, exist_ok=True)
    meshutil.write_ply(os.path.join(outdir, 'material_mesh.ply'), vertices, triangles, normals=normals, colors=_u8(diffuse),
                       extra={'spec': spec.float().contiguous(), 'rough': rough.float().contiguous(), 'material': label})
    names = ['code_%03d' % k for k in range(K)]
    face_src = split['face_src'].long()
    meshutil.write_mtl(os.path.join(outdir, 'material_mesh.mtl'), names, mtl_rows(rows))
    meshutil.write_obj(os.path.join(outdir, 'material_mesh.obj'), vertices, triangles[face_src], split['face_offset'], names, normals=normals)
    fo, vo = split['face_offset'], split['vert_offset']
    areas = face_areas(vertices, triangles[face_src])
    zero = torch.zeros((), dtype=torch.float64, device=vertices.device)
    area = torch.stack([areas[fo[k]: fo[k + 1]].sum() if fo[k + 1] > fo[k] else zero for k in range(K)])
    regions = region_counts(triangles[face_src], label, K)
    if parts:
        wanted = [k for k in range(K) if split['face_count'][k] > 0] if codes is None else [int(k) for k in codes]
        colors = _u8(diffuse)
        for k in wanted:
            if not 0 <= k < K:
                raise ValueError(f'material_mesh.run: codes names {k}, the model has codes 0 .. {K - 1}')
            src = split['vert_src'][vo[k]: vo[k + 1]].long()
            meshutil.write_ply(os.path.join(outdir, names[k] + '.ply'), vertices[src], split['tris_local'][fo[k]: fo[k + 1]],
                               normals=None if normals is None else normals[src], colors=colors[src])
    record = {'n_codes': K, 'n_vertices': int(vertices.shape[0]), 'n_faces': int(triangles.shape[0]), 'branch': branch,
              'smooth': int(smooth), 'self_weight': int(self_weight), 'changed': changed.tolist(), 'dropped_faces': split['dropped'],
              'codes': [{'code': k, 'vertices': split['vert_count'][k], 'faces': split['face_count'][k], 'area': a, 'regions': r}
                        for k, (a, r) in enumerate(zip(area.tolist(), regions.tolist()))]}
    if views is not None:
        record['views'] = write_views(outdir, vertices, triangles, views, diffuse, label, rough)
    with open(os.path.join(outdir, 'material_mesh.json'), 'w') as f:
        json.dump(record, f, indent=1)
    if log is not None:
        log(f"material_mesh: {record['n_faces'] - record['dropped_faces']} faces in "
            f"{sum(1 for c in record['codes'] if c['faces'])} of {K} codes -> {outdir}")
    return record
