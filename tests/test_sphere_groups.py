"""rt_sphere_groups_build / rt_sphere_groups_kept / rt_cast_rays_grouped /
rt_occlude_rays_grouped / rt_cast_camera_grouped on the host (DESIGN.md §3.1j,
§4): the records against the numpy restatement byte for byte, the grouped calls
against the *_accel and the unculled calls word for word, the tie rule among
spheres, the keep test between the exact fp32 sphere tests from below (never
rejects) and an independent float64 line-box clipping from above (not vacuous),
and the argument contract.  No GPU.
"""
import ctypes
import inspect
import shutil
import subprocess

import numpy as np
import pytest

import light_contract as lc
import light_ref as lr
import rays_ref as yr
import sphere_groups_ref as sg
import test_rays as tr

F32 = np.float32


def same(got, want):
    return got.shape == want.shape and got.tobytes() == want.tobytes()


def spheres(pkg, centres, radius):
    c = np.zeros((len(radius), 4), F32)
    c[:, :3] = np.asarray(centres, F32).reshape(-1, 3)
    c[:, 3] = 1.0
    col = np.tile(np.array([0.5, 0.5, 0.5, 255.0], F32), (len(radius), 1))
    return pkg.Scene(c, np.asarray(radius, F32), col)


def random_spheres(pkg, n, seed=7, centre=0.0, spread=(400.0, 300.0, 60.0)):
    rng = np.random.default_rng(seed)
    return spheres(pkg, centre + rng.uniform(-1, 1, (n, 3)) * spread, rng.uniform(0.5, 30.0, n))


# --- 1. the records ---------------------------------------------------------------------------
def test_record_layout(pkg):
    assert pkg.SPHERE_GROUP_DTYPE == sg.group_dtype() and pkg.SPHERE_GROUP_DTYPE.itemsize == 64
    lib = pkg.library()
    for n, g, want in ((0, 8, 0), (1, 8, 1), (8, 8, 1), (9, 8, 2), (300, 3, 100), (7, 1, 7)):
        assert lib.rt_sphere_groups_count(n, g) == want == sg.count(n, g)
    for n, g in ((-1, 8), (4, 0), (4, 9), (4, -1)):
        assert lib.rt_sphere_groups_count(n, g) == -1
    assert lib.rt_sphere_groups_workspace_bytes(0) == 16
    assert lib.rt_sphere_groups_workspace_bytes(5) == 64
    assert lib.rt_sphere_groups_workspace_bytes(-1) == -1


def record_scenes(pkg):
    rng = np.random.default_rng(3)
    base = random_spheres(pkg, 40, 11)
    c, r = base.sphere_origins[:, :3].copy(), base.sphere_radius.copy()
    odd_c, odd_r = c.copy(), r.copy()
    odd_c[3, 1], odd_c[17, 0], odd_c[18, 2] = np.nan, np.inf, -np.inf
    odd_r[5], odd_r[29] = np.nan, np.inf
    signed = r.copy()
    signed[::3] *= -1
    signed[1::5] = 1e-22
    out = {f"scene{i}": pkg.Scene.reference(i) for i in (1, 2, 3)}
    out.update({
        "synthetic": pkg.Scene.synthetic(640, 480, 60, 4, seed=3),
        "config3": pkg.Scene.synthetic(4096, 4096, 256, 64, seed=3, k=4096 / 640),
        "coincident": spheres(pkg, np.repeat(c[:5], 4, 0), np.tile(r[:4], 5)),
        "one_point": spheres(pkg, np.tile([3.0, -4.0, 5.0], (11, 1)), r[:11]),
        "flat_x": spheres(pkg, c * [0, 1, 1] + [7, 0, 0], r),
        "line_z": spheres(pkg, c * [0, 0, 1], r),
        "non_finite": spheres(pkg, odd_c, odd_r),
        "all_non_finite": spheres(pkg, np.full((9, 3), np.nan), r[:9]),
        "signed_and_tiny": spheres(pkg, c, signed),
        "at_1e6": spheres(pkg, c + 1e6, r),
        "zeros": spheres(pkg, np.array([[0.0, -0.0, 0.0], [-0.0, 0.0, -0.0]] * 3), np.zeros(6)),
        "huge": spheres(pkg, rng.uniform(-1, 1, (12, 3)) * 3e38, rng.uniform(0, 3e38, 12)),
    })
    for n in (0, 1, 7, 8, 9, 300):
        out[f"n{n}"] = random_spheres(pkg, n, 100 + n)
    return out


@pytest.mark.parametrize("group_size", [1, 3, 8])
def test_records_equal_the_restatement(pkg, group_size):
    for name, scene in record_scenes(pkg).items():
        got = pkg.build_sphere_groups(scene, group_size)
        want = sg.records(scene.sphere_origins, scene.sphere_radius, group_size)
        assert got.shape == (sg.count(scene.num_spheres, group_size),), name
        assert same(got, want.astype(pkg.SPHERE_GROUP_DTYPE)), name
        if not scene.num_spheres:
            continue
        members = got["member"][got["member"] >= 0]
        assert sorted(members) == list(range(scene.num_spheres)), name  # each sphere once
        assert (got["count"] == (got["member"] >= 0).sum(1)).all(), name
        assert (np.diff(got["member"], axis=1)[got["member"][:, 1:] >= 0] > 0).all(), name
        assert not (np.signbit(got["lo"]) & (got["lo"] == 0)).any(), name  # a zero bound is +0
        assert not (np.signbit(got["hi"]) & (got["hi"] == 0)).any(), name
    got = pkg.build_sphere_groups(record_scenes(pkg)["non_finite"], group_size)
    bad = np.isin(got["member"], [3, 5, 17, 18, 29]).any(1)
    assert bad.any() and (got["rmax"][bad] == np.inf).all() and (got["lo"][bad] == -np.inf).all()
    assert np.isfinite(got["rmax"][~bad]).all() and (got["hi"][bad] == np.inf).all()
    # the non-finite spheres sort behind every finite one
    assert set(got["member"][-(-5 // group_size):].ravel()) >= {3, 5, 17, 18, 29}


def test_the_box_holds_its_members_and_equal_keys_fall_back_to_index_order(pkg):
    scene = record_scenes(pkg)["signed_and_tiny"]
    got = pkg.build_sphere_groups(scene, 3)
    c = scene.sphere_origins[:, :3].astype(np.float64)
    r = np.abs(scene.sphere_radius.astype(np.float64))
    for rec in got:
        m = rec["member"][:rec["count"]]
        assert (rec["lo"] <= (c[m] - r[m, None]).min(0)).all()
        assert (rec["hi"] >= (c[m] + r[m, None]).max(0)).all()
        assert rec["rmax"] == r[m].max().astype(F32)
    one = pkg.build_sphere_groups(record_scenes(pkg)["one_point"], 3)
    assert one["member"][:, :3].ravel()[:11].tolist() == list(range(11))
    # neighbours along the curve, not along the index: the groups' boxes are
    # much smaller than the scene
    scene = random_spheres(pkg, 300, 5)
    got = pkg.build_sphere_groups(scene, 8)
    size = (got["hi"] - got["lo"]).max(1)
    assert np.median(size) < 0.45 * 800


# --- 2. grouped = culled = unculled, word for word -----------------------------------------
def compare(pkg, scene, rays, label="", group_sizes=(8, 3), restate=True):
    accel = pkg.build_accel(scene)
    want, want_tri = pkg.cast_rays(rays, scene, triangles=True)
    occ = pkg.occlude_rays(rays, scene)
    assert same(pkg.cast_rays_accel(rays, scene, accel), want), f"{label} accel"
    for group_size in group_sizes:
        groups = pkg.build_sphere_groups(scene, group_size)
        for order in (groups, groups[::-1].copy()):  # in whatever order the groups come
            got, tri = pkg.cast_rays_grouped(rays, scene, accel, order, triangles=True)
            assert same(got, want) and same(tri, want_tri), f"{label} cast {group_size}"
            assert same(pkg.occlude_rays_grouped(rays, scene, accel, order), occ), \
                f"{label} occluded {group_size}"
        assert same(pkg.cast_rays_grouped(rays, scene, accel, groups), want), label
        for segment in (False, True):
            assert same(pkg.sphere_groups_kept(rays, scene, groups, segment),
                        sg.kept_count(groups, rays, segment)), f"{label} kept {segment}"
    if restate:
        hits, ref_tri = sg.cast(scene, accel, groups, rays)
        assert same(want, hits.astype(pkg.HIT_DTYPE)) and same(want_tri, ref_tri), \
            f"{label} restated cast"
        assert same(occ, sg.occlude(scene, accel, groups, rays)), f"{label} restated occlusion"
    return accel, groups, want, occ


@pytest.mark.parametrize("name", ["base", "twins", "sphere_tie", "spheres_only", "cubes_only",
                                  "empty"])
def test_random_rays(pkg, name):
    scene = tr.scenes(pkg)[name]
    small = dict(box=((0, 64), (0, 48), (-70, 20)))
    rays = yr.random_rays(scene, 768, 31, **(dict(small, skips=[-1, 2]) if name == "twins" else
                                             small if name == "sphere_tie" else {}))
    accel, groups, hits, occ = compare(pkg, scene, rays, name)
    if name in ("empty", "cubes_only"):
        assert len(groups) == 0
    if name == "empty":  # and with NULL arrays
        null = type(scene.as_c())()
        out, p = np.zeros(len(rays), pkg.HIT_DTYPE), rays.astype(pkg.RAY_DTYPE)
        assert pkg.library().rt_cast_rays_grouped(p.ctypes.data, len(p), ctypes.byref(null), None,
                                                  None, 0, out.ctypes.data, None) == 0
        assert (out["object"] == -1).all()


def test_many_spheres(pkg):
    scene = pkg.Scene.synthetic(640, 480, 70, 6, seed=13)
    rays = yr.random_rays(scene, 1500, 37, box=((0, 640), (0, 480), (-120, 60)))
    rays = np.concatenate([rays, pkg.camera_rays(pkg.Camera.reference(), 640, 480)[::9, ::11]
                           .reshape(-1)])
    accel, groups, hits, occ = compare(pkg, scene, rays, "many", restate=False)
    nc = scene.num_cubes
    assert (hits["object"] >= nc).sum() >= 100 and 50 <= occ.sum()
    kept = pkg.sphere_groups_kept(rays, scene, groups)
    assert kept.mean() < 0.5 * len(groups)  # a cull, not a keep-everything
    assert (kept[hits["object"] >= nc] >= 1).all()


@pytest.mark.parametrize("name", ["mirror", "kinds"])
def test_the_light_pass_scenes(pkg, oracle, name):
    import reflect_ref as rr
    import shadow_ref as sr
    if name == "mirror":
        scene = rr.mirror_scene(pkg)
        hits, r = rr.restated(oracle, "mirror", scene, rr.MIRROR_W, rr.MIRROR_H)
        rays, on = yr.bounce_rays(hits, r)
    else:
        scene = sr.kinds_scene(pkg, lights=(sr.KINDS_LIGHT, (-30, 64, 40, 1)))
        hits, r = lr.restated(sr.shadow_ref, oracle, "shadow_kinds", scene, sr.KINDS_W, sr.KINDS_H)
        rays, where = yr.facing_segments(oracle, scene, hits, 0)
    rays = rays[::7]  # (the restatement of the walks runs per cube and per group)
    accel, groups, got, occ = compare(pkg, scene, rays, name)
    if name == "mirror":
        assert (got["object"] >= 0).sum() >= 100 and (got["object"] == -1).sum() >= 100
    else:
        assert 100 <= occ.sum() <= len(rays) - 100


@pytest.mark.parametrize("name", yr.EDGE_NAMES)
def test_edge_rays(pkg, name):
    scene = lr.base(pkg)
    rays = yr.edge_rays(scene)[name]
    accel, groups, hits, occ = compare(pkg, scene, rays, name)
    kept = pkg.sphere_groups_kept(rays, scene, groups)
    fields = np.stack([rays[f] for f in ("ox", "oy", "oz", "dx", "dy", "dz")])
    odd = ~np.isfinite(fields).all(0)
    if name in ("nan", "inf"):  # the fallback: every group
        assert odd.sum() >= 72 and (kept[odd] == len(groups)).all()
    if name == "zero_direction":
        still = (fields[3:] == 0).all(0)  # a = 0: the fallback
        assert still.sum() >= 30 and (kept[still] == len(groups)).all()
    if name == "inside_a_sphere":
        assert (kept >= 1).all()


W, H, BAND = tr.W, tr.H, tr.BAND


@pytest.mark.parametrize("camera", ["reference", "pinhole", "generic"])
@pytest.mark.parametrize("rows", [None, BAND], ids=["frame", "band"])
def test_cast_camera(pkg, camera, rows):
    scene = lr.base(pkg)
    cam = {"reference": pkg.Camera.reference(),
           "pinhole": pkg.Camera.pinhole((30, 20, 90), (32, 24, -40), (0, -1, 0), 50.0, W, H),
           "generic": pkg.Camera(**dict(yr.generic_camera(1), o0=(30.0, 20.0, 40.0)))}[camera]
    accel, groups = pkg.build_accel(scene), pkg.build_sphere_groups(scene, 2)
    want, want_tri = pkg.cast_camera(cam, scene, W, H, rows, triangles=True)
    assert (want["object"] >= 0).sum() >= 50 and (want["object"] == -1).sum() >= 20
    assert same(pkg.cast_camera_accel(cam, scene, accel, W, H, rows), want)
    got, tri = pkg.cast_camera_grouped(cam, scene, accel, groups, W, H, rows, triangles=True)
    assert same(got, want) and same(tri, want_tri)
    assert same(pkg.cast_camera_grouped(cam, scene, accel, groups, W, H, rows), want)
    rays = pkg.camera_rays(cam, W, H, rows)
    assert same(pkg.cast_rays_grouped(rays, scene, accel, groups), want)


# --- 3. the tie rule ------------------------------------------------------------------------
@pytest.mark.parametrize("copies", [2, 3])
def test_identical_spheres_in_different_groups(pkg, copies):
    """Identical spheres at indices 1, 4 (and 6) among others, one group each:
    the smallest index wins whatever order the groups come in."""
    base = random_spheres(pkg, 8, 21, spread=(40.0, 30.0, 20.0))
    c, r = base.sphere_origins[:, :3].copy(), base.sphere_radius.copy()
    twins = [1, 4, 6][:copies]
    c[twins], r[twins] = c[1], r[1]
    scene = spheres(pkg, c, r)
    rng = np.random.default_rng(5)
    o = c[1] + np.array([0, 0, 200.0]) + rng.uniform(-1, 1, (400, 3)) * 5
    d = c[1] + rng.uniform(-1, 1, (400, 3)) * r[1] * 0.9 - o
    rays = yr.make_rays(o.T.astype(F32), d.T.astype(F32), -1)
    want = pkg.cast_rays(rays, scene)
    assert (want["object"] == 1).sum() >= 100 and not np.isin(want["object"], twins[1:]).any()
    accel = pkg.build_accel(scene)
    groups = pkg.build_sphere_groups(scene, 1)
    where = {int(g["member"][0]): i for i, g in enumerate(groups)}
    assert len({where[t] for t in twins}) == copies
    rng2 = np.random.default_rng(9)
    for trial in range(6):
        order = groups[rng2.permutation(len(groups))] if trial else groups[::-1].copy()
        assert same(pkg.cast_rays_grouped(rays, scene, accel, order), want)
    # and with the first twin left out, the next one
    rays["skip"] = 1
    want = pkg.cast_rays(rays, scene)
    assert (want["object"] == 4).sum() >= 100
    assert same(pkg.cast_rays_grouped(rays, scene, accel, groups[::-1].copy()), want)


def test_a_cube_with_the_same_t_still_wins(pkg, oracle):
    """tests/test_rays.py's tie: the quadratic's s0 and a triangle's (float)td
    are the same float; cubes come first."""
    import reflect_ref as rr
    scene = tr.scenes(pkg)["sphere_tie"]
    hits, r = rr.restated(oracle, "reflect_sphere_tie", scene, 64, 48)
    y, x = rr.TIE_PIXEL
    tie = yr.make_rays([a[y, x] for a in r.p], [a[y, x] for a in r.R], hits["object"][y, x])
    rays = tie.reshape(1).astype(pkg.RAY_DTYPE)
    accel, groups = pkg.build_accel(scene), pkg.build_sphere_groups(scene, 1)
    want = pkg.cast_rays(rays, scene)
    assert want["object"][0] == 0 and scene.num_cubes >= 1
    ok, s0, far = rr.sphere_sf(yr.origins(rays), yr.directions(rays), scene.sphere_origins[0],
                               scene.sphere_radius[0])
    assert ok[0] and s0[0].view(np.uint32) == want["t"][0].view(np.uint32)
    assert same(pkg.cast_rays_grouped(rays, scene, accel, groups), want)


# --- 4. never rejects -------------------------------------------------------------------------
def perpendicular(u, rng):
    w = np.cross(u, rng.normal(size=u.shape))
    return w / np.linalg.norm(w, axis=1, keepdims=True)


def axes(rng, n):
    """Unit vectors, half of them along an axis."""
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    k = rng.integers(0, 3, n)
    e = np.eye(3)[k] * rng.choice([-1.0, 1.0], n)[:, None]
    w = np.eye(3)[(k + rng.integers(1, 3, n)) % 3] * rng.choice([-1.0, 1.0], n)[:, None]
    axis = rng.random(n) < 0.5
    return np.where(axis[:, None], e, u), np.where(axis[:, None], w, perpendicular(u, rng))


def family_tangent(c, r, rng, n, segment, ends=(0.5,)):
    """Rays aimed at perpendicular offsets r (1 +- 1e-8 .. 1e-1) from the
    centre, from origins 10 .. 1e7 radii away; a segment's tangent point at
    parameter `ends`."""
    u, w = axes(rng, n)
    eps = 10.0 ** rng.uniform(-8, -1, n) * rng.choice([-1.0, 1.0], n)
    dist = abs(r) * 10.0 ** rng.uniform(1, 7, n)
    o = c + w * (abs(r) * (1 + eps))[:, None] - u * dist[:, None]
    if segment:
        d = u * (dist / rng.choice(ends, n))[:, None]
    else:
        d = u * (10.0 ** rng.uniform(-1, 3, n))[:, None]
    return o, d


def family_surface_ends(c, r, rng, n):
    """Segments towards the sphere that end at 0.999, 1 and 1.001 of the
    distance to its surface."""
    u, _ = axes(rng, n)
    dist = abs(r) * 10.0 ** rng.uniform(0.1, 5, n)
    o = c - u * dist[:, None]
    aim = c + perpendicular(u, rng) * (abs(r) * rng.uniform(0, 0.9, n))[:, None] - o
    surface = np.linalg.norm(aim, axis=1) - abs(r)  # (about: the aim is off the centre)
    aim /= np.linalg.norm(aim, axis=1, keepdims=True)
    return o, aim * (surface * rng.choice([0.999, 1.0, 1.001, 1.5], n))[:, None]


def family_away(c, r, rng, n):
    u, w = axes(rng, n)
    o = c + u * (abs(r) * 10.0 ** rng.uniform(0.001, 4, n))[:, None] + w * abs(r) * 0.3
    return o, u * (10.0 ** rng.uniform(-1, 3, n))[:, None]


def family_on_and_inside(c, r, rng, n):
    u, w = axes(rng, n)
    depth = rng.choice([1.0, 1.0, 1 - 1e-6, 1 + 1e-6, 0.5, 0.0], n)
    o = c + u * (abs(r) * depth)[:, None]
    d = rng.normal(size=(n, 3)) * (10.0 ** rng.uniform(-1, 2, n))[:, None]
    return o, d


def family_lengths(c, r, rng, n):
    u, w = axes(rng, n)
    o = c + w * (abs(r) * rng.uniform(0, 1.2, n))[:, None] - u * (abs(r) * 20)
    return o, u * (10.0 ** rng.uniform(-4, 30, n))[:, None]


def family_fallback(c, r, rng, n):
    u, w = axes(rng, n)
    o = c + w * (abs(r) * rng.uniform(0, 3.0, n))[:, None] - u * (abs(r) * 20)
    d = u * (10.0 ** rng.choice([-44.0, -40.0, -30.0, -10.0, 19.0, 25.0, 38.0], n))[:, None]
    d[::7] = 0.0
    d[1::11, 0], o[2::13, 1], d[3::17, 2] = np.nan, np.inf, -np.inf
    return o, d


FAMILIES = {
    "tangent_casts": lambda c, r, g, n: family_tangent(c, r, g, n, False),
    "tangent_segments": lambda c, r, g, n: family_tangent(c, r, g, n, True, (0.5, 0.999, 1.001)),
    "surface_ends": family_surface_ends,
    "away": family_away,
    "on_and_inside": family_on_and_inside,
    "lengths": family_lengths,
    "fallback": family_fallback,
}
N = 4000  # rays per sphere and family


def never_rejects_scene(pkg):
    """Spheres of ordinary, tiny, huge and negative radius, some far from the
    frame of the others."""
    c = np.array([[10, 20, -30], [18, 25, -34], [-40, 0, 5], [300, -200, 90], [1e6, 1e6, -1e6],
                  [12, 22, -28], [0, 0, 0], [5e4, 2e4, -7e4]], np.float64)
    r = np.array([7.5, 3.0, 1e-22, 60.0, 250.0, -4.0, 1e-3, 3e4])
    return spheres(pkg, c, r), c.astype(F32).astype(np.float64), r.astype(F32).astype(np.float64)


def group_of(groups, s):
    return int(np.nonzero((groups["member"] == s).any(1))[0][0])


def rays_of(o, d):
    with np.errstate(all="ignore"):
        return yr.make_rays(o.T.astype(F32), d.T.astype(F32), -1)


def dropped(scene, groups, rays, s, segment, c):
    """Rays on which sphere `s` is accepted and its group is not kept (with
    the margin's constant `c`)."""
    got = sg.accepted(scene.sphere_origins[s], scene.sphere_radius[s], rays, segment)
    keep = sg.kept(yr.origins(rays), yr.directions(rays), groups[group_of(groups, s)], segment, c)
    return got & ~keep, got


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("group_size", [1, 3])
def test_never_rejects(pkg, family, group_size):
    """Every accepted sphere lies in a kept group, as a cast and as a segment;
    the library's counts are the restatement's, and its grouped calls the
    unculled calls, on the same rays."""
    scene, c, r = never_rejects_scene(pkg)
    groups = pkg.build_sphere_groups(scene, group_size)
    accel = pkg.build_accel(scene)
    rng = np.random.default_rng(hash(family) % 1000 + group_size)
    accepted = 0
    for s in range(len(r)):
        rays = rays_of(*FAMILIES[family](c[s], r[s], rng, N))
        for segment in (False, True):
            bad, got = dropped(scene, groups, rays, s, segment, sg.C)
            assert not bad.any(), (s, segment, rays[bad][:3])
            accepted += int(got.sum())
            assert same(pkg.sphere_groups_kept(rays, scene, groups, segment),
                        sg.kept_count(groups, rays, segment)), (s, segment)
        assert same(pkg.cast_rays_grouped(rays, scene, accel, groups), pkg.cast_rays(rays, scene))
        assert same(pkg.occlude_rays_grouped(rays, scene, accel, groups),
                    pkg.occlude_rays(rays, scene))
    if family not in ("away", "fallback"):
        assert accepted >= 1000, accepted
    if family == "fallback":
        o, d = yr.origins(rays), yr.directions(rays)
        assert all(sg.in_fallback(o, d, g).mean() > 0.5 for g in groups)


def test_the_family_has_teeth():
    """With the margin's constant 0 the restatement drops accepted spheres on
    the near-tangent family: the margin is needed, and the family can tell."""
    class S:  # the restatement needs no library
        sphere_origins = np.array([[10, 20, -30, 1]], F32)
        sphere_radius = np.array([7.5], F32)
    groups = sg.records(S.sphere_origins, S.sphere_radius, 1)
    rng = np.random.default_rng(2)
    o, d = family_tangent(np.array([10.0, 20.0, -30.0]), 7.5, rng, 40000, False)
    rays = rays_of(o, d)
    bad, got = dropped(S, groups, rays, 0, False, 0.0)
    assert bad.sum() >= 1 and got.sum() >= 1000
    bad, _ = dropped(S, groups, rays, 0, False, sg.C)
    assert not bad.any()


# --- 5. not vacuous ---------------------------------------------------------------------------
def test_a_clear_miss_is_rejected(pkg):
    """A group whose box, grown by 1 % of (far-corner distance + rmax), the
    float64 clipping of the whole line misses is rejected: the one shipped
    ground, exact by construction for a margin constant <= 1e-2."""
    scene = random_spheres(pkg, 60, 31)
    groups = pkg.build_sphere_groups(scene, 4)
    rays = yr.random_rays(scene, 3000, 77, box=((-900, 900), (-700, 700), (-300, 300)))
    o, d = yr.origins(rays), yr.directions(rays)
    O = np.stack(o, 1).astype(np.float64)
    D = np.stack(d, 1).astype(np.float64)
    rejected = total = 0
    for segment in (False, True):
        per_group = []
        for rec in groups:
            lo, hi = rec["lo"].astype(np.float64), rec["hi"].astype(np.float64)
            far = np.maximum(np.abs(O - lo), np.abs(O - hi)).sum(1)
            clear = ~sg.line_hits_box(O, D, lo, hi, 0.01 * (far + float(rec["rmax"])))
            keep = sg.kept(o, d, rec, segment)
            assert not sg.in_fallback(o, d, rec).any()
            assert not (clear & keep).any()
            rejected += int(clear.sum())
            total += len(clear)
            per_group.append(keep)
        assert same(pkg.sphere_groups_kept(rays, scene, groups, segment),
                    np.sum(per_group, 0).astype(np.int32))
    assert rejected > 0.5 * total


def test_config3_keeps_few_groups(pkg):
    """The bench's scene: on 8192 sampled reference-camera rays at most 6 of
    the 32 groups are kept on average (a keep-everything gives 32)."""
    scene = pkg.Scene.synthetic(4096, 4096, 256, 64, seed=3, k=4096 / 640)
    assert scene.num_spheres == 256
    groups = pkg.build_sphere_groups(scene)
    assert len(groups) == 32
    rng = np.random.default_rng(1)
    ys, xs = rng.integers(0, 4096, 8192), rng.integers(0, 4096, 8192)
    cam = pkg.Camera.reference()
    d = pkg.camera_rays(cam, 4, 1)[0, 0]  # origin (x, y, 0), one direction for every pixel
    rays = yr.make_rays((xs.astype(F32), ys.astype(F32), np.zeros(8192, F32)),
                        (d["dx"], d["dy"], d["dz"]), -1).astype(pkg.RAY_DTYPE)
    for i in range(8):
        y, x = int(ys[i]), int(xs[i])
        assert same(rays[i:i + 1], pkg.camera_rays(cam, 4096, 4096, (y, y + 1))[0, x:x + 1])
    kept = pkg.sphere_groups_kept(rays, scene, groups)
    print("config 3: groups kept per ray", kept.mean())
    assert kept.mean() <= 6.0
    hit = pkg.cast_rays(rays, scene)
    assert (kept[hit["object"] >= scene.num_cubes] >= 1).all()
    accel = pkg.build_accel(scene)
    assert same(pkg.cast_rays_grouped(rays, scene, accel, groups), hit)


# --- 6. the argument contract -----------------------------------------------------------------
class Args(tr.Args):
    def __init__(self, pkg):
        super().__init__(pkg)
        self.accel = pkg.build_accel(self.scene)
        self.groups = pkg.build_sphere_groups(self.scene, 2)
        self.kept = np.zeros(64, np.int32)
        self.out = np.zeros(len(self.groups), pkg.SPHERE_GROUP_DTYPE)
        self.ws = np.zeros(64 + 8 * self.scene.num_spheres, np.uint8)
        p = lambda a: a.ctypes.data  # noqa: E731
        for a in (self.accel, self.groups, self.out, self.ws):
            assert p(a) % 16 == 0
        g, sc, ng = self.good, ctypes.byref(self.sc), len(self.groups)
        self.good = {
            "build": dict(scene=sc, group_size=2, out=p(self.out)),
            "build_device": dict(scene=sc, group_size=2, out=p(self.out), ws=p(self.ws),
                                 ws_bytes=len(self.ws)),
            "kept": dict(rays=g["cast"]["rays"], n=8, scene=sc, groups=p(self.groups),
                         num_groups=ng, segment=0, count=p(self.kept)),
            "cast": dict(rays=g["cast"]["rays"], n=8, scene=sc, accel=p(self.accel),
                         groups=p(self.groups), num_groups=ng, hits=p(self.hits),
                         tri=p(self.tri)),
            "occlude": dict(rays=g["cast"]["rays"], n=8, scene=sc, accel=p(self.accel),
                            groups=p(self.groups), num_groups=ng, occ=p(self.occ)),
            "cast_camera": dict(cam=ctypes.byref(self.cam), scene=sc, accel=p(self.accel),
                                groups=p(self.groups), num_groups=ng, width=4, rb=1, re=3,
                                hits=p(self.hits), tri=p(self.tri)),
        }
        self.symbols = {"build": "rt_sphere_groups_build", "build_device": "rt_sphere_groups_build",
                        "kept": "rt_sphere_groups_kept", "cast": "rt_cast_rays_grouped",
                        "occlude": "rt_occlude_rays_grouped",
                        "cast_camera": "rt_cast_camera_grouped"}
        self.host = ("build", "kept", "cast", "occlude", "cast_camera")
        self.device = ("build_device", "cast", "occlude", "cast_camera")


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_bad_arguments_are_refused(pkg, device):
    """What the *_accel calls refuse, and a NULL or misaligned groups / out /
    workspace, a workspace too small, a group_size outside 1..8, a num_groups
    that is no count of this scene's spheres, a NULL count, a segment other
    than 0 or 1; the device entry points refuse the same before any HIP call
    (behind a context that is never used)."""
    a = Args(pkg)
    ctx = ctypes.c_void_p(a.hits.ctypes.data) if device else None
    bad = pkg.RT_ERR_INVALID_ARG
    ns = a.scene.num_spheres
    counts = {sg.count(ns, g) for g in range(1, 9)}
    for name in (a.device if device else a.host):
        good = a.good[name]
        if device:
            fn = getattr(a.lib, a.symbols[name] + "_device")
            assert fn(None, *good.values(), None) == bad, name
        else:
            assert a.call(name) == 0, name
        refused = tr.refusals(a, name)
        refused += [(k, v) for k in ("accel", "groups", "out", "ws", "count") if k in good
                    for v in (None, good[k] + 8, good[k] + 4)]
        refused = [(k, good[k] + 2 if k == "count" and v else v) for k, v in refused]
        if "segment" in good:
            refused += [("segment", 2), ("segment", -1)]
        if "group_size" in good:
            refused += [("group_size", v) for v in (0, 9, -1, 1 << 30)]
        if "ws_bytes" in good:
            refused += [("ws_bytes", v) for v in (0, -1, 16 + 8 * ns - 1)]
        if "num_groups" in good:
            refused += [("num_groups", v) for v in (-1, 0, ns + 1, 1 << 30) if v not in counts]
        for key, value in refused:
            assert a.call(name, ctx, **{key: value}) == bad, (name, key, value)
        if "width" in good:
            for width, rb, re in lc.SHAPES:
                assert a.call(name, ctx, width=width, rb=rb, re=re) == bad, (name, width, rb, re)
            assert a.call(name, ctx, width=1 << 24, rb=0, re=1 << 24) == pkg.RT_ERR_UNSUPPORTED
        elif "n" in good:
            assert a.call(name, ctx, n=tr.MAX_RAYS + 1) == pkg.RT_ERR_UNSUPPORTED
    # every count of this scene's spheres is a num_groups (the records decide the rest)
    assert len(counts) >= 3
    # no spheres: NULL groups, out and workspace are fine, also on the device
    # (nothing is launched); num_groups must be 0
    none = pkg.Scene().as_c()
    assert a.call("build", scene=ctypes.byref(none), out=None) == 0
    assert a.call("build_device", ctypes.c_void_p(a.hits.ctypes.data), scene=ctypes.byref(none),
                  out=None, ws=None, ws_bytes=0) == 0
    free = a.rays.copy()
    free["skip"] = -1
    rays = free.ctypes.data
    empty = dict(rays=rays, scene=ctypes.byref(none), accel=None, groups=None, num_groups=0)
    assert a.call("cast", **empty) == 0
    assert a.call("cast", **dict(empty, num_groups=1)) == bad
    a.kept[:] = 7
    assert a.call("kept", rays=rays, scene=ctypes.byref(none), groups=None, num_groups=0) == 0
    assert not a.kept[:8].any() and (a.kept[8:] == 7).all()
    # n == 0 writes nothing
    a.hits["object"] = 7
    assert a.call("cast", n=0) == 0 and a.call("cast", ctypes.c_void_p(a.hits.ctypes.data), n=0) == 0
    assert (a.hits["object"] == 7).all()


def test_a_foreign_member_index_is_no_sphere(pkg):
    """A stale record is not detected, but nothing is read through an index
    outside the scene."""
    scene = lr.base(pkg)
    rays = yr.random_rays(scene, 64, 3)
    accel, groups = pkg.build_accel(scene), pkg.build_sphere_groups(scene, 2)
    groups["member"][:, 1] = scene.num_spheres + 7
    groups["member"][0, 0] = -5
    groups["count"][:] = 100
    got = pkg.cast_rays_grouped(rays, scene, accel, groups)
    assert got.shape == rays.shape
    pkg.occlude_rays_grouped(rays, scene, accel, groups)


def test_python_names(pkg):
    lib = pkg.library()
    header = (lc.REPO / "include" / "rt_hip.h").read_text()
    for symbol in ("rt_sphere_groups_build", "rt_sphere_groups_build_device",
                   "rt_sphere_groups_kept", "rt_cast_rays_grouped", "rt_occlude_rays_grouped",
                   "rt_cast_camera_grouped", "rt_cast_rays_grouped_device",
                   "rt_occlude_rays_grouped_device", "rt_cast_camera_grouped_device"):
        assert symbol in pkg.EXPORTED_SYMBOLS and hasattr(lib, symbol) and f"int {symbol}(" in header
    for symbol in ("rt_sphere_groups_count", "rt_sphere_groups_workspace_bytes"):
        assert symbol in pkg.EXPORTED_SYMBOLS and hasattr(lib, symbol) and f" {symbol}(" in header
    assert "typedef struct rt_sphere_group" in header and lib.rt_abi_version() == 1
    params = {
        (pkg, "build_sphere_groups"): ["scene", "group_size"],
        (pkg, "sphere_groups_kept"): ["rays", "scene", "groups", "segment"],
        (pkg, "cast_rays_grouped"): ["rays", "scene", "accel", "groups", "triangles"],
        (pkg, "occlude_rays_grouped"): ["rays", "scene", "accel", "groups"],
        (pkg, "cast_camera_grouped"): ["camera", "scene", "accel", "groups", "width", "height",
                                       "rows", "triangles"],
        (pkg.RayTracer, "build_sphere_groups_device"): ["self", "device_scene", "group_size",
                                                        "out_ptr", "workspace_ptr",
                                                        "workspace_bytes", "stream"],
        (pkg.RayTracer, "cast_rays_grouped_device"): ["self", "rays_ptr", "n", "device_scene",
                                                      "accel_ptr", "groups_ptr", "num_groups",
                                                      "hits_ptr", "triangles_ptr", "stream"],
        (pkg.RayTracer, "occlude_rays_grouped_device"): ["self", "rays_ptr", "n", "device_scene",
                                                         "accel_ptr", "groups_ptr", "num_groups",
                                                         "out_ptr", "stream"],
        (pkg.RayTracer, "cast_camera_grouped_device"): ["self", "camera", "device_scene",
                                                        "accel_ptr", "groups_ptr", "num_groups",
                                                        "width", "rows", "hits_ptr",
                                                        "triangles_ptr", "stream"],
    }
    for (owner, name), want in params.items():
        if owner is pkg:
            assert name in pkg.__all__
        assert list(inspect.signature(getattr(owner, name)).parameters) == want, name
    assert "SPHERE_GROUP_DTYPE" in pkg.__all__
    assert inspect.signature(pkg.build_sphere_groups).parameters["group_size"].default == 8
    scene = lr.base(pkg)
    rays = yr.random_rays(scene, 8, 3)
    with pytest.raises(ValueError):
        pkg.cast_rays_grouped(rays, scene, pkg.build_accel(scene), np.zeros(3, np.float32))
    with pytest.raises(pkg.RtError):  # no count of this scene's spheres
        pkg.cast_rays_grouped(rays, scene, pkg.build_accel(scene),
                              np.zeros(scene.num_spheres + 3, pkg.SPHERE_GROUP_DTYPE))
    with pytest.raises(pkg.RtError):
        pkg.build_sphere_groups(scene, 9)


# --- 7. under the sanitizers ---------------------------------------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_sphere_groups_arguments_under_sanitizers(tmp_path):
    """tests/sphere_groups_args_check.cpp, a program of its own over the host
    sources, under AddressSanitizer + UndefinedBehaviorSanitizer."""
    csrc = lc.REPO / "opencl-ray-tracer_amd" / "csrc"
    exe = tmp_path / "sphere_groups_args_check"
    subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-std=c++17",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{lc.REPO / 'include'}", "-o", str(exe),
                    str(lc.REPO / "tests" / "sphere_groups_args_check.cpp"),
                    str(csrc / "rt_sphere_groups.cpp"), str(csrc / "rt_accel.cpp"),
                    str(csrc / "rt_light.cpp"), str(csrc / "rt_args.cpp"), "-lm"],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "sphere groups args check ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
