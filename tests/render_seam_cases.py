"""Designed scenes that put the RENDER kernels on the scene sizes at which the code changes kernels, list sizes, step counts
or capacities (csrc/rt_lists.hpp, rt_trace.hpp, rt_dense.hpp, the path choice in rt_tracer.hpp); test_render_seam_cases.py
checks without a device that every case holds what it promises, test_gpu_render_seams.py renders them.  A helper, not a test.
Everything is deterministic and needs no device.

Random scenes never sit on those sizes with a known number of candidates per tile.  These scenes are made of

  covers     large triangles, wound towards the camera, that EVERY ray of EVERY tile of the frame hits: a conservative
             classifier has to keep each of them in every list of every level.  Cover k lies at its own depth with a small tilt
             of its own (colour = |normal|: the frame shows which one won); one of them, the case's `winner`, lies behind all
             the others at D_WIN -- under the reference's farthest-hit rule it is what every ray sees.
  outs       small triangles at |x| >= 60, |z| <= 6 that no LINE of the camera's ray family meets (the reference accepts
             negative t: "behind the camera" would not do; a 70 degree camera at the origin reaches |x| < 11 there).  They face
             the camera in planes that pass the lens at a distance, so every level of the classification drops them.
  partials   small triangles given by a rectangle of the frame: a `rival` behind the winner (D_RIVAL), so that the tiles on
             its edge have no certain winner and the tiles inside it another one; an `occluder` in front of the covers (D_OCC),
             which only the nearest-hit rule shows.  Where they lie is decided per tile by brute force (partial_tiles()).
  twins      a record and a bit-identical copy at the next index, in the edge layout with different packed vertex normals:
             with smooth_normals only the colour says which of the two won (the first one scanned has to).
  filler     scenes.random_triangles at the remaining indices of the large scenes that are not about counts.

so the number of candidates of every tile is known by construction: the covers, plus the partials that reach the tile."""
import zlib

import numpy as np

f32 = np.float32
CAMERA = dict(angles=(0.0, 0.0), fov=70.0, focal=6.0, aperture=0.05)
TAN = float(np.tan(np.radians(35.0)))
SPP = 5                                          # a remainder at K = 2 and at K = 4
# wide: 5 x 6 macro tiles of 128 x 64 (> 16: the super level); column: 2 x 9 of them on rows short enough for an oracle of 65 537 triangles
FRAMES = {"a": (96, 40), "b": (72, 40), "tall": (96, 136), "wide": (640, 328), "column": (136, 520)}
D_NEAR, D_FAR, D_WIN, D_RIVAL, D_OCC = 2.0, 6.0, 7.5, 9.0, 1.25
RECTS = {"rival": (0.08, 0.10, 0.66, 0.92), "occluder": (0.70, 0.15, 0.97, 0.80)}     # fractions of the frame: x0, y0, x1, y1
LENS = np.array([(0.0, 0.0)] + [(np.cos(a), np.sin(a)) for a in np.arange(8) * np.pi / 4], np.float64)
N_COVERS = 20                                    # of a small-scene case: three passes of region_level2
NO_LIST = 0xFFFFFFFF


def tiles_of(frame):
    W, H = FRAMES[frame] if isinstance(frame, str) else frame
    return (H + 7) // 8, (W + 7) // 8


# ------------------------------------------------------------------------------------------------------------ geometry
def cover(depth, tx, ty):
    """A triangle over the whole frustum of every frame of FRAMES at z ~ -depth, counter-clockwise seen from the camera."""
    d = float(depth)
    return [[-6 * d, -3 * d, -d * (1 - tx - ty)], [6 * d, -3 * d, -d * (1 + tx - ty)], [0.0, 9 * d, -d * (1 + 3 * ty)]]


def unproject(frame, u, v, depth):
    W, H = FRAMES[frame]
    return [(2.0 * u / W - 1.0) * TAN * (W / H) * depth, (1.0 - 2.0 * v / H) * TAN * depth, -depth]


def partial(frame, kind):
    """The triangle (x0, y1), (x1, y1), (x0, y0) of the kind's rectangle of the frame, at the kind's depth."""
    W, H = FRAMES[frame]
    x0, y0, x1, y1 = RECTS[kind]
    d = D_RIVAL if kind == "rival" else D_OCC
    return [unproject(frame, x0 * W, y1 * H, d), unproject(frame, x1 * W, y1 * H, d), unproject(frame, x0 * W, y0 * H, d)]


def outs(n, seed):
    """(n, 3, 3): small triangles at |x| in [60, 80], |y| <= 5, z in [-6, -2], facing the camera like the covers.  (Not near
    z = 0: a triangle whose PLANE passes through the lens has det' ~ 0 for every ray, and no interval test can drop it.)"""
    r = np.random.default_rng(seed)
    side = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    c = np.stack([side * r.uniform(60, 80, n), r.uniform(-5, 5, n), r.uniform(-6, -2, n)], axis=1)
    shape = np.array([[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [0.0, 1.0, 0.0]])
    tri = c[:, None, :] + r.uniform(0.05, 0.15, (n, 1, 1)) * shape[None]
    tri[:, :, 2] += r.uniform(-0.02, 0.02, (n, 3))
    return tri


def rays_of_tile(frame, tx, ty, pixels=None):
    """(origins, directions) in float64 of the tile's pixels (all 64 in the image, or `pixels`) x LENS"""
    W, H = FRAMES[frame]
    if pixels is None:
        pixels = [(x, y) for y in range(ty * 8, min(ty * 8 + 8, H)) for x in range(tx * 8, min(tx * 8 + 8, W))]
    px = np.array(pixels, np.float64)
    d = np.stack([(2 * (px[:, 0] + 0.5) / W - 1) * TAN * (W / H), (1 - 2 * (px[:, 1] + 0.5) / H) * TAN, -np.ones(len(px))], axis=1)
    F = CAMERA["focal"] * d / np.linalg.norm(d, axis=1, keepdims=True)
    o = np.concatenate([LENS * CAMERA["aperture"], np.zeros((len(LENS), 1))], axis=1)
    O = np.repeat(o[None], len(px), 0).reshape(-1, 3)
    return O, (F[:, None, :] - o[None]).reshape(-1, 3)


def lines_meet(O, D, tri):
    """which of the lines O + t D (any t) pass through the triangle: plain float64 Moeller-Trumbore without the culling"""
    v0, v1, v2 = (np.asarray(v, np.float64) for v in tri)
    e1, e2 = v1 - v0, v2 - v0
    pv = np.cross(D, e2)
    det = pv @ e1
    tv = O - v0
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.einsum("ij,ij->i", tv, pv) / det
        v = np.einsum("ij,ij->i", D, np.cross(tv, e1)) / det
    return (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1)


def partial_tiles(frame, tri):
    """(tiles_y, tiles_x) int8: 0 = no ray of the tile's 64 pixels x LENS meets the triangle, 2 = every ray does, 1 = some do"""
    ny, nx = tiles_of(frame)
    out = np.zeros((ny, nx), np.int8)
    for ty in range(ny):
        for tx in range(nx):
            m = lines_meet(*rays_of_tile(frame, tx, ty), tri)
            out[ty, tx] = 2 if m.all() else 1 if m.any() else 0
    return out


def clear_of(status, ring=1):
    """tiles with no ray on the triangle in the tile itself or within `ring` tiles of it"""
    s = np.pad(status, ring) != 0
    near = np.zeros_like(status, bool)
    for dy in range(2 * ring + 1):
        for dx in range(2 * ring + 1):
            near |= s[dy:dy + status.shape[0], dx:dx + status.shape[1]]
    return ~near


# ------------------------------------------------------------------------------------------------------------ the cases
def _case(name, group, n, covers, winner=None, partials=None, frame="a", options=None, env=None, twins=None, filler=None,
          nearest=False, promise=None):
    covers = sorted(set(int(i) for i in covers))
    partials = dict(partials or {})                                   # index -> kind
    assert (twins is None or twins + 1 in covers) and all(0 <= i < n for i in covers) and (winner is None or winner in covers) and not set(partials) & set(covers), name
    return dict(name=name, group=group, n=n, covers=covers, winner=winner, partials=partials, frame=frame, camera=CAMERA, spp=SPP,
                options=dict(options or {}), env=dict(env or {}), twins=twins, filler=filler, nearest=nearest,
                promise=dict(promise or {}))


def small_covers(n, c=N_COVERS):
    """c cover indices of a small scene: the indices on both sides of every step of 32 and 64 the scene has, the first eight
    after index 1 and the last eight before n - 2 (1 and n - 2 stay free for the rival, 10 for the occluder), then evenly"""
    free = {1, n - 2, 10}
    want = [0, n - 1, 63, 64, 31, 32, 65, 127, 128, 129, 191, 192, 193, 255, 256]
    want += list(range(2, 10)) + list(range(n - 10, n - 2)) + [int(round(k * (n - 1) / 37.0)) for k in range(38)]
    out = []
    for i in want:
        if 0 <= i < n and i not in free and i not in out and len(out) < c:
            out.append(i)
    return out


def _small_cases():
    cases = []
    sizes = (31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257)
    for k, n in enumerate(sizes):
        opts = {"bin_list": 288} if n == 257 else {}
        bin_list = 288 if n == 257 else max(32, (n + 31) // 32 * 32)
        winners = [w for w in (0, 63, 64, n - 1) if w < n]
        for j, w in enumerate(dict.fromkeys(winners)):
            # the rival before the winner (index 1) or after it (n - 2), alternating over the table; what cannot be is swapped
            rival = 1 if (j + k) % 2 == 0 else n - 2
            if w == 0:
                rival = n - 2
            if rival == w:
                rival = 1
            frame = "tall" if (n, w) == (193, 64) else ("a", "b")[(k + j) % 2]
            cov = small_covers(n)
            if w not in cov:
                cov[-1] = w
            cases.append(_case("small_n%d_w%d_r%d" % (n, w, rival), "small", n, cov, w, {rival: "rival", 10: "occluder"}, frame, opts,
                               nearest=(j == 0), promise=dict(path="small", bin_list=bin_list, k=2 if n <= 128 else 4)))
    # lists exactly full: every record a cover, n = bin_list; 65 for the gather loop's second trip; 960: the 10-bit fields
    for n, w, opts in ((32, 17, {}), (64, 0, {}), (65, 64, {}), (256, 255, {}), (960, 959, {"bin_list": 960})):
        cases.append(_case("small_full_n%d" % n, "small", n, range(n), w, None, "b" if n == 64 else "a", opts,
                           promise=dict(path="small", bin_list=opts.get("bin_list", max(32, (n + 31) // 32 * 32)), k=2 if n <= 128 else 4,
                                        full=n != 65)))
    # region candidates: covers + outs, the pair kernel (n = 32) and the region kernel (n = 100)
    for n in (32, 100):
        for c in (4, 5, 8, 9, 16, 17):
            cov = small_covers(n, c)
            cases.append(_case("small_n%d_cand%d" % (n, c), "small", n, cov, cov[-1], None, "b" if c % 2 else "a",
                               promise=dict(path="small", bin_list=32 if n == 32 else 128, k=2)))
    return cases


def _scan_cases():
    cases = []
    for n, chunk_req, c in ((1023, 0, 1024), (1024, 0, 1024), (1025, 0, 1024), (2049, 0, 1024), (37, 1, 1), (4096, 5000, 4096), (4097, 5000, 4096)):
        opts = dict(no_binning=True, **({"lds_chunk": chunk_req} if chunk_req else {}))
        seam = [i for i in (0, c - 1, c, c + 1, 2 * c - 1, 2 * c, n - 1, n // 2) if 0 <= i < n]
        prom = dict(path="scan", lds_chunk=c, lds_bytes=min(n, c) * 36, k=2 if n <= 128 else 4)
        for w in dict.fromkeys(i for i in (c - 1, c, n - 1) if 0 <= i < n):
            cases.append(_case("scan_n%d_c%d_w%d" % (n, c, w), "scan", n, seam, w, {5: "rival"} if n > 64 else {3: "rival"},
                               "b" if w == c else "a", opts, nearest=(w == n - 1), promise=prom))
        if c < n:                                                      # twins across the seam: both are the farthest cover
            cases.append(_case("scan_n%d_c%d_twins" % (n, c), "scan", n, seam, c - 1, None, "a", dict(opts, smooth_normals=True),
                               twins=c - 1, promise=prom))
    return cases


def _runs(*spans):
    return [i for a, b in spans for i in range(a, b)]


def _large_cases():
    P = lambda path, **kw: dict(path=path, k=4, **kw)
    cases = [
        # SmallLists -> Classify at 257 with the default list: every record kept (n_src = 257: the second block step has one
        # valid lane), and 20 covers among outs without the macro lists
        _case("large_n257_all", "large", 257, range(257), 256, promise=P("classify", stats=True)),
        _case("large_n257_nomacro", "large", 257, small_covers(257), 256, {1: "rival", 10: "occluder"}, "b", dict(no_macro_bins=True),
              promise=P("classify")),
        # the block list exactly full (1024 kept) and one more (the waves walk the macro tile's list instead)
        _case("large_n1100_block1024", "large", 1100, _runs((0, 500), (538, 1024), (1062, 1100)), 1099, promise=P("classify", stats=True)),
        _case("large_n1100_block1025", "large", 1100, _runs((0, 500), (537, 1024), (1062, 1100)), 1099, promise=P("classify", stats=True)),
        # ... and without the macro lists the waves walk the SCENE: 191 covers in the first three steps, 64 in the fourth --
        # the round closes at L - 1 = 191
        _case("large_n1100_midstep", "large", 1100, _runs((0, 191), (192, 1026)), 1025, None, "a", dict(no_macro_bins=True),
              promise=P("classify", stats=True)),
        # ClassifyForms: block list 448 | 449; at 449 the waves walk the scene: 64 + 19 = L - 1 = 83 covers in two steps
        _case("large_n4096_forms448", "large", 4096, _runs((0, 83), (128, 493)), 492, None, "a", dict(no_macro_bins=True),
              promise=P("forms", stats=True)),
        _case("large_n4096_forms449", "large", 4096, _runs((0, 83), (128, 494)), 493, None, "a", dict(no_macro_bins=True),
              promise=P("forms", stats=True)),
        # DenseLists: 84 covers = wave_cap in every tile, and the rival makes 85 where it reaches
        _case("large_n4096_dense84", "large", 4096, [48 * i + 7 for i in range(83)] + [4095], 4095, promise=P("dense", wave_full=True)),
        _case("large_n4096_dense85", "large", 4096, [48 * i + 7 for i in range(83)] + [4095], 4095, {2000: "rival"}, "b",
              promise=P("dense", wave_full=True)),
        # the macro list exactly full and one more (RT_MI355X_MACRO_CAP)
        _case("large_n300_macro40", "large", 300, [7 * i + 3 for i in range(39)] + [299], 299, env={"RT_MI355X_MACRO_CAP": "40"},
              promise=P("classify", stats=True)),
        _case("large_n300_macro41", "large", 300, [7 * i + 3 for i in range(40)] + [299], 299, env={"RT_MI355X_MACRO_CAP": "40"},
              promise=P("classify", stats=True)),
    ]
    # path and level switches: random filler behind three covers and an occluder
    for n in (2047, 2048, 4095, 4096, 50000, 50001, 65536, 65537):
        frame = "wide" if n in (2047, 2048) else "column" if n >= 65536 else "a"
        path = "dense" if 4096 <= n <= 50000 else "classify"
        cases.append(_case("large_n%d_filler" % n, "large", n, (0, n // 2, n - 1), None, {7: "occluder"}, frame,
                           filler=n, nearest=n in (4095, 4096), promise=P(path, bands=frame != "a" or n >= 50000)))
    return cases


CASES = _small_cases() + _scan_cases() + _large_cases()
BY_NAME = {c["name"]: c for c in CASES}


def depths(case):
    """cover index -> (depth, tx, ty): the winner behind, the others at distinct depths in an order that is not the upload order"""
    cov = [i for i in case["covers"] if i != case["winner"]]
    c = len(cov)
    order = np.random.default_rng(zlib.crc32(case["name"].encode())).permutation(c)
    step = (D_FAR - D_NEAR) / max(c, 1)
    t = step / 15.0 / D_FAR                                            # the tilt moves a cover by less than a quarter of a step
    out = {i: (D_NEAR + step * int(order[k]), t * np.cos(2.4 * k), t * np.sin(2.4 * k)) for k, i in enumerate(cov)}
    if case["winner"] is not None:
        out[case["winner"]] = (D_WIN, 0.02, -0.015)
    if case["twins"] is not None:
        out[case["twins"] + 1] = out[case["twins"]]
    return out


def triangles(case, without=None):
    """(n, 3, 3) float32 vertices; without: that record replaced by an out (the indices of the others stay)"""
    n = case["n"]
    if case["filler"] is not None:
        from raytracertest_amd import scenes
        tris = scenes.random_triangles(n, case["filler"])[:, :3].reshape(n, 3, 3).astype(np.float64)
    else:
        tris = outs(n, zlib.crc32(case["name"].encode()) & 0xFFFF)
    for i, (d, tx, ty) in depths(case).items():
        tris[i] = cover(d, tx, ty)
    for i, kind in case["partials"].items():
        tris[i] = partial(case["frame"], kind)
    if without is not None:
        tris[without] = outs(1, 99)[0]
    return tris.astype(f32)


def scene(case, without=None, swap_twins=False):
    """(rows, edge layout?) as UploadScene / UploadSceneEdges take them"""
    tris = triangles(case, without)
    rows = np.zeros((3 * case["n"], 4), f32)
    rows[:, :3] = tris.reshape(-1, 3)
    if case["twins"] is None:
        return rows, False
    from raytracertest_amd import meshes
    nrm = np.random.default_rng(5).normal(size=(3 * case["n"], 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    a = case["twins"]
    nrm[3 * a:3 * a + 3] = (0.0, 0.6, 0.8)                             # the twins differ in nothing but these
    nrm[3 * a + 3:3 * a + 6] = (0.8, 0.0, 0.6)
    if swap_twins:
        nrm[3 * a:3 * a + 3], nrm[3 * a + 3:3 * a + 6] = nrm[3 * a + 3:3 * a + 6].copy(), nrm[3 * a:3 * a + 3].copy()
    return meshes.to_edge_format(rows, normals=nrm.astype(f32)), True


def designated(case):
    """the record whose removal has to change the frame: the winner (the first twin: its copy takes over, with other
    normals)"""
    if case["winner"] is not None:
        return case["winner"]
    d = depths(case)
    return max(d, key=lambda i: d[i][0])                              # (scenes with filler: the deepest cover)


_STATUS = {}


def tile_counts(case):
    """(lo, hi, clear, status): per tile the fewest and the most candidates a conservative list may hold -- the covers, plus the partials
    that certainly / possibly reach it; clear: the tiles with no partial in them or near them (lo == hi == the covers)"""
    ny, nx = tiles_of(case["frame"])
    lo = np.full((ny, nx), len(case["covers"]), np.int32)                # (a twin's copy is a cover of its own)
    hi = lo.copy()
    clear = np.ones((ny, nx), bool)
    status = {}
    for i, kind in case["partials"].items():
        if (case["frame"], kind) not in _STATUS:
            _STATUS[case["frame"], kind] = partial_tiles(case["frame"], partial(case["frame"], kind))
        st = _STATUS[case["frame"], kind]
        status[i] = st
        # a conservative list may hold a partial next to where its rays are: the rival lies near the focal distance; the occluder
        # at D_OCC is out of focus by 0.04 (3 pixels of the tall frame) and the family's lens is a box: two tiles
        ring = 2 if kind == "occluder" else 1
        lo += st != 0
        hi += ~clear_of(st, ring)
        clear &= clear_of(st, ring)
    return lo, hi, clear, status


def classify_walk(keep, L):
    """what trace_kernel's classify() does with the keep flags of the triangles it walks, in steps of 64: a step that does not fit
    opens the next round -> the candidates of every round of one walk over the list"""
    keep = np.asarray(keep, bool)
    base, rounds = 0, []
    while base < keep.size or not rounds:
        count = 0
        while base < keep.size and count < L:
            k = int(keep[base:base + 64].sum())
            if count + k > L:
                break
            count += k
            base += 64
        rounds.append(count)
    return rounds


def classify_rounds(keep, L):
    """(candidates, rounds) of one walk"""
    r = classify_walk(keep, L)
    return sum(r), len(r)
