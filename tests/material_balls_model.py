"""The float64 numpy statement of the material-ball renderer (include/vqn_material_balls.h; csrc/material_balls.hip): geometry, shading,
averaging, background, the 8-bit transfer and the sheet tiling, written from reading the reference's brdf/renderer.py (SphereRenderer,
gen_light_xyz, load_light), its util/microfacet.py:9-89 and vq_nfr.py:694-723, :830-833.  The sample grid, the foreground test and the
argument of the height's square root are evaluated in float32, one rounded operation each as the header states them, so the mask is
bit-equal to the kernel's; everything after that is float64.  Helpers only, no tests."""
import numpy as np

CAM_DIST = 10.0
DEFAULT_ROT = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])
EPS = 1e-6                       # tf.linalg.l2_normalize's floor on the squared norm, as the shading code applies it


def gen_light_xyz(h, w, radius=1e2):
    lat_step, lng_step = np.pi / (h + 2), 2 * np.pi / (w + 2)
    lats = np.linspace(np.pi / 2 - lat_step, -np.pi / 2 + lat_step, h)
    lngs = np.linspace(np.pi - lng_step, -np.pi + lng_step, w)
    lngs, lats = np.meshgrid(lngs, lats)
    xyz = np.stack([radius * np.cos(lats) * np.cos(lngs), radius * np.cos(lats) * np.sin(lngs), radius * np.sin(lats)], -1)
    sin_colat = np.sin(np.pi / 2 - lats)
    return xyz, 4 * np.pi * sin_colat / np.sum(sin_colat)


def load_light(name, h=16):
    """the two synthetic probes of the reference's load_light"""
    if name == 'white':
        return np.ones((h, 2 * h, 3))
    if name == 'point':
        env = np.zeros((h, 2 * h, 3))
        i, j, d = -h // 4, -int(2 * h * 7 / 8), 2
        env[(i - d):(i + d), (j - d):(j + d), :] = 1
        return env
    raise ValueError(name)


def sps_of(spp):
    sps = int(round(np.sqrt(spp)))
    assert sps * sps == spp
    return sps


def grid(ims, spp):
    """float32 [ims * sps]: the sample coordinates of one axis"""
    f = np.float32
    sps = sps_of(spp)
    n = ims * sps
    a = f(1) / f(sps + 1)
    step = (f(ims) - f(2) * a) / f(n - 1) if n > 1 else f(0)
    return (a + np.arange(n, dtype=np.float32) * step) / f(ims)


def samples(ims, spp, radius=0.4):
    """-> dx, dy float32 [n, n] (column, row offsets from the centre), fg bool [n, n], hz2 float32 [n, n] (radius^2 - d2, clamped at 0)"""
    f = np.float32
    d = grid(ims, spp) - f(0.5)
    dx, dy = np.broadcast_to(d[None, :], (d.size, d.size)), np.broadcast_to(d[:, None], (d.size, d.size))
    d2 = dx * dx + dy * dy
    assert d2.dtype == np.float32
    fg = np.sqrt(d2) <= f(radius)
    hz2 = np.maximum(f(radius) * f(radius) - d2, f(0))
    return dx, dy, fg, hz2


def _normalize(x):
    return x / np.sqrt(np.maximum((x * x).sum(-1, keepdims=True), EPS))


def _div_no_nan(a, b):
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(b == 0, 0.0, a / np.where(b == 0, 1.0, b))


def geometry(ims, spp, radius=0.4, cam_rot=None):
    """the foreground samples, row-major: -> (fg bool [n, n], xyz [S, 3], normal [S, 3] (turned toward the camera), cam [3]), float64"""
    rot = DEFAULT_ROT if cam_rot is None else np.asarray(cam_rot, np.float64).reshape(3, 3)
    dx, dy, fg, hz2 = samples(ims, spp, radius)
    p_cam = np.stack([dx[fg].astype(np.float64), -dy[fg].astype(np.float64), np.sqrt(hz2[fg].astype(np.float64))], -1)
    xyz = p_cam @ rot.T
    cam = rot @ np.array([0.0, 0.0, CAM_DIST])
    normal = _normalize(xyz)
    v = _normalize(cam[None] - xyz)
    flip = (normal * v).sum(-1) < 0
    normal = np.where(flip[:, None], -normal, normal)
    return fg, xyz, normal, cam


def _g1(c, a2):
    c = np.clip(c, 0.0, 1.0)
    return _div_no_nan(2 * c, c + np.sqrt(np.abs(a2 + (1 - a2) * c * c)))


def shade(xyz, normal, cam, materials, lights, lxyz, areas, parts=False):
    """xyz, normal [S, 3], materials [M, 7], lights [P, L, 3] -> the plain sums over the lights [S, M, P, 3] (no gamma, no clip); with
    parts also (diffuse, glossy) of the same shape and t_min [S]: the smallest 1 - (h.n)^2 over the front-lit lights of a sample"""
    materials, lights = np.asarray(materials, np.float64), np.asarray(lights, np.float64)
    lxyz, areas = np.asarray(lxyz, np.float64).reshape(-1, 3), np.asarray(areas, np.float64).reshape(-1)
    l = _normalize(lxyz[None] - xyz[:, None])                         # [S, L, 3]
    v = _normalize(_normalize(cam[None] - xyz))
    n = _normalize(normal)
    cos_l = (l * normal[:, None]).sum(-1)                             # vq_nfr.py:702
    front = cos_l > 0
    h = _normalize(l + v[:, None])
    om5 = (1 - np.clip((h * v[:, None]).sum(-1), 0.0, 1.0)) ** 5      # [S, L]
    cm2 = np.clip((h * n[:, None]).sum(-1), 0.0, 1.0) ** 2
    l_dot_n = (l * n[:, None]).sum(-1)
    v_dot_n = (v * n).sum(-1)                                         # [S]
    w = (cos_l * areas[None] * front)[:, :, None, None] * lights.transpose(1, 0, 2)[None]        # [S, L, P, 3]
    w_sum = w.sum(1)
    S, M = xyz.shape[0], materials.shape[0]
    out = np.zeros((S, M, lights.shape[0], 3))
    diff, gloss = np.zeros_like(out), np.zeros_like(out)
    for m in range(M):
        albedo, f0, rough = materials[m, :3], materials[m, 3:6], materials[m, 6]
        a2 = (rough ** 2) ** 2
        F = f0[None, None] + (1 - f0[None, None]) * om5[:, :, None]                               # [S, L, 3]
        D = _div_no_nan(a2, np.pi * (cm2 * (a2 - 1) + 1) ** 2)                                    # [S, L]
        G = _g1(l_dot_n, a2) * _g1(v_dot_n, a2)[:, None]
        glossy = _div_no_nan(F * (G * D)[:, :, None], (4 * np.abs(l_dot_n) * np.abs(v_dot_n)[:, None])[:, :, None] * np.ones(3))
        gloss[:, m] = np.einsum('slc,slpc->spc', glossy, w)
        diff[:, m] = (albedo / np.pi)[None, None] * w_sum
        out[:, m] = gloss[:, m] + diff[:, m]
    if not parts:
        return out
    t_min = np.where(front, 1 - cm2, np.inf).min(1)
    return out, diff, gloss, t_min


def finish(rgb, gamma=None):
    """the plain sums -> displayed linear values: (rgb * g0) ^ g1 when gamma is given, then the clip to [0, 1]"""
    if gamma is not None:
        rgb = np.power(rgb * gamma[0], gamma[1])
    return np.clip(rgb, 0.0, 1.0)


def average(sample_img, spp):
    """[n, n, ...] per-sample values -> [ims, ims, ...]: the mean over the sps x sps samples of a pixel (SphereRenderer.render)"""
    sps = sps_of(spp)
    acc = 0.0
    for i in range(sps):
        for j in range(sps):
            acc = acc + sample_img[i::sps, j::sps]
    return acc / (sps * sps)


def pixel_fg_count(ims, spp, radius=0.4):
    """int [ims, ims]: the foreground samples of every pixel"""
    return np.rint(average(samples(ims, spp, radius)[2].astype(np.float64), spp) * spp).astype(np.int64)


def render(materials, lights, lxyz, areas, ims, spp, radius=0.4, cam_rot=None, white_bg=True, gamma=None, details=False):
    """-> float64 [M, P, ims, ims, 3]; details: also t_min [ims, ims], the smallest 1 - (h.n)^2 over the front-lit lights of the
    pixel's foreground samples (inf where it has none): where it is tiny, a mirror-like lobe points at a light and f32 cannot resolve
    the lobe's argument"""
    fg, xyz, normal, cam = geometry(ims, spp, radius, cam_rot)
    M, P = np.asarray(materials).shape[0], np.asarray(lights).shape[0]
    img = np.full(fg.shape + (M, P, 3), 1.0 if white_bg else 0.0)
    t_img = np.full(fg.shape, np.inf)
    if xyz.shape[0]:
        out, _, _, t_min = shade(xyz, normal, cam, materials, lights, lxyz, areas, parts=True)
        img[fg] = finish(out, gamma)
        t_img[fg] = t_min
    res = average(img, spp).transpose(2, 3, 0, 1, 4)
    if not details:
        return res
    sps = sps_of(spp)
    return res, t_img.reshape(ims, sps, ims, sps).min((1, 3))


def linear2srgb(x):
    """img.py:142-186 in float32, as the device conversion evaluates it; the bytes are the truncation of 255 times this"""
    t = np.clip(np.asarray(x, np.float32), np.float32(0), np.float32(1))
    return np.where(t <= np.float32(0.0031308), t * np.float32(12.92),
                    np.float32(1.055) * np.power(t, np.float32(1 / 2.4)) - np.float32(0.055)).astype(np.float32)


def sheet(u8, order, rows, cols, white_bg=True):
    """u8 [M, P, ims, ims, 3] bytes -> [P, rows * ims, cols * ims, 3]: ball order[i] at cell (i // cols, i % cols), the rest background"""
    M, P, ims = u8.shape[:3]
    order = list(range(M)) if order is None else list(order)
    assert len(order) <= rows * cols
    out = np.full((P, rows * ims, cols * ims, 3), 255 if white_bg else 0, np.uint8)
    for i, m in enumerate(order):
        r, c = i // cols, i % cols
        out[:, r * ims:(r + 1) * ims, c * ims:(c + 1) * ims] = u8[m]
    return out
