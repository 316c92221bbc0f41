"""Every launch sequence render_common (csrc/pt_api.hip) can choose, times every shading feature, against the CPU oracle bit for bit.

A FORM is a context created under a set of flags and knobs: the sequences of the fused schedule over a tree staged in LDS (one launch; a
separate looping pass behind the segmented or the dense hand-over; queue-fed passes in between, counted or polled; the looping pass as
tail_kernel), the split schedule, and both schedules over a tree in global memory with 16-bit and with 32-bit stack entries -- the
bounce_kernel<false, ...> instances of pt_bounce_g16.hip / pt_bounce_g32.hip run only under PT_SPLIT=0, which no other test sets.
A FEATURE is a scene of about 24 spheres that shows one thing the shading code does: alpha-tested constant alpha, every material map with
rotations, alpha tested against a map, a lat-long and a cube environment under a transform, sphere-light DI, DI with a textured emitter,
the denoiser outputs.  The 32-bit forms render the same spheres among filler that brings the tree to 32 800 leaves.

Every case renders its view three times (the third frame takes its primary candidates from the beam lists where the form has them) at
1 and 3 spp and once without Russian roulette, and must equal the oracle's frame in every bit of every pixel, ray for ray.  That the form
under test is the one that ran is read from the frame's launch counts (set_profiling: PtStats counts launches by kind; the counts are
those of render_common's loops) and from where pt_build_accel put the tree.  The CPU tests at the top show that the scenes do show their
feature and that their paths live long enough for the looping and the queue-fed passes to have work."""
import copy
import os

import numpy as np
import pytest

from util import bits, context_under, count_mismatch, render_rested

gpu = pytest.mark.gpu

BOUNCES = 6
N_BIG = 32800  # the 32-bit forms: with_tree_walk takes 32-bit stack entries from 32767 nodes
DLSS_RR, REBLUR = 1, 2  # abi_types.DENOISER_*
KNOBS = ("PT_SPLIT", "PT_FUSE_LOOP", "PT_SEG", "PT_INLINE2_MIN_SLOTS", "PT_TAIL_AFTER", "PT_TAIL_THRESHOLD", "PT_LOOP_USE_TAIL", "PT_RAY_REPLACEMENT",
         "PT_WIDE", "PT_BEAMS", "PT_COOP_WALK", "PT_NO_ADAPTIVE_GRID")
NO_LDS, SPLIT_KERNELS = 1, 8  # abi_types.PT_FLAG_NO_LDS_SCENE, PT_FLAG_SPLIT_KERNELS

# form -> (knobs, flags, where the tree lives, the sequence, sample counts the sequence exists at)
#   queue: the counted queue-fed passes are a 1-spp sequence (at spp > 1 the knobs select nothing: the looping pass carries the frame);
#   polled: the polled ones an spp > 1 sequence
FORMS = {
    "fused": ({}, 0, "lds", "fused", (1, 3)),
    "separate": ({"PT_FUSE_LOOP": "0"}, 0, "lds", "separate", (1, 3)),
    "queue": ({"PT_INLINE2_MIN_SLOTS": "100000000", "PT_TAIL_AFTER": "2"}, 0, "lds", "queue", (1,)),
    "dense": ({"PT_SEG": "0"}, 0, "lds", "separate", (1, 3)),
    "polled": ({"PT_TAIL_THRESHOLD": "64"}, 0, "lds", "polled", (3,)),
    "loop_tail": ({"PT_LOOP_USE_TAIL": "1"}, 0, "lds", "separate", (1, 3)),
    "split": ({}, SPLIT_KERNELS, "lds", "split", (1, 3)),
    "g16_split_dyn_wide": ({}, NO_LDS, "g16", "split", (1, 3)),
    "g16_split_plain_binary": ({"PT_RAY_REPLACEMENT": "0", "PT_WIDE": "0"}, NO_LDS, "g16", "split", (1, 3)),
    "g16_fused": ({"PT_SPLIT": "0"}, NO_LDS, "g16", "fused", (1, 3)),
    "g16_separate": ({"PT_SPLIT": "0", "PT_FUSE_LOOP": "0"}, NO_LDS, "g16", "separate", (1, 3)),
    "g32_split": ({}, 0, "g32", "split", (1, 3)),
    "g32_fused": ({"PT_SPLIT": "0"}, 0, "g32", "fused", (1, 3)),
}
FEATURES = ("plain", "maps", "alpha_map", "latlong", "cube", "di", "di_textured", "denoiser")


def expected_launches(sequence, spp, di):
    """(traverse-kind, shade, looping) launches of one frame, or None where the count depends on the queue sizes -- from render_common:
    fused: the primary pass alone.  separate: the primary pass, then the looping pass (kind 3).  queue: PT_TAIL_AFTER = 2 compacting passes
    between them.  split, 1 spp: primary, shade(0), then traverse(k) / shade(k) for k = 1 .. tail_after = 4, then the tail; spp > 1: the lagged
    poll sees the size of queue 1 (far below the 262144-ray threshold, never zero in these scenes) after shade(2).  The split schedule's DI
    estimate is one more traverse-kind launch."""
    if sequence == "fused":
        return 1, 0, 0
    if sequence == "separate":
        return 1, 0, 1
    if sequence == "queue":
        return 3, 0, 1
    if sequence == "split":
        return (5 if spp == 1 else 3) + (1 if di else 0), 5 if spp == 1 else 3, 1
    return None


# ------------------------------------------------------------------------------------------------------------------ the feature scenes
def _extras(dxrs, rng, k):
    """k small glossy / glass spheres scattered over lit_scene's floor, so that its scenes have about as many spheres as the others"""
    s = np.zeros(k, dtype=dxrs.SPHERE_DTYPE)
    s["cx"], s["cz"], s["r"] = rng.uniform(-4.0, 4.0, k), rng.uniform(-4.5, 3.0, k), rng.uniform(0.15, 0.3, k)
    s["cy"] = -0.5 + s["r"]
    m = dxrs.types.default_material(k)
    m["BaseColor"][:, :3] = rng.uniform(0.5, 1.0, (k, 3))
    m["Roughness"] = rng.choice([0.0, 0.1, 0.5], k)
    m["Metallic"] = rng.choice([0.0, 1.0], k)
    m["Transmission"] = np.where(m["Metallic"] > 0, 0.0, rng.choice([0.0, 1.0], k))
    return s, m


# seeds of the generators' scenes that meet the conditions of test_the_scenes_show_their_feature (chosen with the oracle, which checks them)
PLAIN_SEED, MAPS_SEED, ALPHA_SEED, ENV_SEED, DI_SEED = 1013, 7001, 21, 9100, 6
_scenes = {}


def scene_of(dxrs, host, feature, big=False):
    """-> dict(spheres, materials, sd, textures, di, w, h, camera position, frame): the feature's scene, made by the generators of the
    feature's own test module.  big: the same spheres first, then procedural filler (tiny spheres over 400 x 400 units, as in the 32 800-sphere
    tests of test_sharc_ex.py) up to N_BIG."""
    if feature == "denoiser":
        feature = "maps"
    if (feature, big) in _scenes:
        return _scenes[(feature, big)]
    from dxrs_amd import textures as T
    small_sd = host.scene(dxrs.host.SCENE_SMALL)[2]
    ts, di, pos, look_at, size = None, False, (0.0, 0.5, -12.0), None, (96, 64)
    if feature == "plain":
        from test_gpu_fuzz import random_scene
        s, m = random_scene(dxrs, np.random.default_rng(PLAIN_SEED), 24)
        assert (m["AlphaMode"] != 0).sum() >= 3  # (the seed is one whose scene has constant-alpha spheres)
        sd, size = small_sd, (97, 61)
    elif feature == "maps":
        from test_textures import make_textured_scene
        s, m, ts = make_textured_scene(dxrs, np.random.default_rng(MAPS_SEED), 24, 1)
        sd = small_sd
    elif feature == "alpha_map":
        from test_alpha import alpha_scene
        s, m, sd, ts, _ = alpha_scene(dxrs, host, ALPHA_SEED, True)
        pos, size = (0.5, 0.6, -2.5), (97, 61)  # (close to the spheres: enough paths go on past depth 2)
    elif feature in ("latlong", "cube"):
        from test_environment_map import random_rotation, set_cube, set_env
        from test_gpu_coop_walk import glass_scene
        rng = np.random.default_rng(ENV_SEED)
        s, m = glass_scene(dxrs, rng)
        ts = T.TextureSet(len(s))
        if feature == "latlong":
            sd = set_env(small_sd, ts.add_hdr_image(T.sky_latlong(128, 64, seed=3)), rng.normal(size=(3, 3)))  # (not orthonormal: normalised after)
        else:
            sd = set_cube(small_sd, ts.add_cube([rng.uniform(0, 4, (5, 5, 4)).astype(np.float32) for _ in range(6)]), random_rotation(rng))
            size = (97, 61)
        pos, look_at = (0.0, 0.8, -14.0), (0.0, 0.0, -3.0)
    else:
        from test_direct_illumination import lit_scene
        textured = feature == "di_textured"
        s, m = lit_scene(dxrs, n_lights=1 if textured else 3, glass=True)
        es, em = _extras(dxrs, np.random.default_rng(DI_SEED), 24 - len(s))
        s, m = np.concatenate([s, es]), np.concatenate([m, em])
        if textured:  # (the two-tone emissive map of test_direct_illumination's _textured_emitter_scene, on the one emitter)
            ts = T.TextureSet(len(s))
            img = np.zeros((8, 16, 4), dtype=np.uint8)
            img[..., 3] = 255
            img[:, :8, :3] = 255
            ts.assign(6, dxrs.types.TEXTURE_MAP_EMISSIVE_COLOR, ts.add_image(img, srgb=False))
            size = (97, 61)
        sd, di, pos = small_sd, True, (0.0, 1.5, -7.0)
    if big:
        fs, fm, _ = host.scene(dxrs.host.SCENE_PROCEDURAL, seed=0, count=N_BIG)
        k = N_BIG - len(s)
        n_hero = len(s)
        s, m = np.concatenate([s, fs[:k]]), np.concatenate([m, fm[:k]])
        if ts is not None:
            wide = T.TextureSet(N_BIG)
            wide.images = ts.images
            wide.maps[:n_hero], wide.rotations[:n_hero] = ts.maps, ts.rotations
            ts = wide
    frame = 3 + FEATURES.index(feature)
    _scenes[(feature, big)] = dict(spheres=s, materials=m, sd=sd, textures=ts, di=di, w=size[0], h=size[1], pos=pos, look_at=look_at, frame=frame)
    return _scenes[(feature, big)]


def _camera(host, sc):
    return host.camera(sc["w"], sc["h"], position=sc["pos"], look_at=sc["look_at"], jitter_index=sc["frame"])


def _settings(dxrs, sc, spp, rr, bounces=BOUNCES, di=None):
    return dxrs.types.graphics_settings(sc["w"], sc["h"], frame_index=sc["frame"], bounces=bounces, spp=spp, rr=rr, di=sc["di"] if di is None else di)


_oracle_cache = {}


def oracle_frame(dxrs, host, oracle, feature, big, spp, rr, bounces=BOUNCES, without=False):
    """The oracle's (frame, stats), rendered once per key.  without: the same frame with the feature taken away."""
    if feature == "denoiser":
        feature = "maps"
    key = (feature, big, spp, rr, bounces, without)
    if key not in _oracle_cache:
        sc = scene_of(dxrs, host, feature, big)
        m, sd, ts, di = sc["materials"], sc["sd"], sc["textures"], sc["di"]
        if without:
            if feature in ("plain", "alpha_map"):
                m = m.copy()
                m["AlphaMode"] = 0
            elif feature in ("maps", "di_textured"):
                ts = None
            elif feature in ("latlong", "cube"):
                ts, sd = None, copy.copy(host.scene(dxrs.host.SCENE_SMALL)[2])
                sd.EnvironmentLightColor[0], sd.EnvironmentLightColor[1], sd.EnvironmentLightColor[2], sd.EnvironmentLightColor[3] = 0.7, 0.8, 1.1, 1.0
            else:
                di = False
        _oracle_cache[key] = oracle.render(sc["spheres"], m, sd, _camera(host, sc), _settings(dxrs, sc, spp, rr, bounces, di), threads=8, textures=ts)
    return _oracle_cache[key]


@pytest.mark.parametrize("feature", FEATURES[:-1])  # (the denoiser frames render the scene of "maps")
def test_the_scenes_show_their_feature(dxrs, host, oracle, feature):
    """CPU, the oracle alone.  Taking the feature away changes at least 5 % of the pixels; at least 5 % of the paths go beyond depth 2, where
    the looping pass, the tail and the queue-fed passes work (rays at depth d = rays(Bounces = d) - rays(Bounces = d - 1); shadow rays are the
    same in both); at 3 spp the rays at depth 1 outnumber three times the polled form's 64-entry threshold (the queue after the primary pass
    holds an entry for every pixel with a sample left to trace, so no fewer than one sample's depth-1 rays)."""
    sc = scene_of(dxrs, host, feature)
    pixels = sc["w"] * sc["h"]
    img, _ = oracle_frame(dxrs, host, oracle, feature, False, 1, True)
    bare, _ = oracle_frame(dxrs, host, oracle, feature, False, 1, True, without=True)
    changed = count_mismatch(img, bare)
    print(f"{feature}: {changed} of {pixels} pixels change without the feature")
    assert changed >= 0.05 * pixels
    if feature == "di_textured":  # ... and DI itself shows, not only the emitter's map
        sc_m, sd, ts = sc["materials"], sc["sd"], sc["textures"]
        no_di, _ = oracle.render(sc["spheres"], sc_m, sd, _camera(host, sc), _settings(dxrs, sc, 1, True, di=False), threads=8, textures=ts)
        assert count_mismatch(img, no_di) >= 0.05 * pixels
    for spp in (1, 3):
        deep = oracle_frame(dxrs, host, oracle, feature, False, spp, True)[1].rays - oracle_frame(dxrs, host, oracle, feature, False, spp, True, bounces=2)[1].rays
        print(f"{feature}: {deep} rays beyond depth 2 of {pixels * spp} paths at {spp} spp")
        assert deep > 0.05 * pixels * spp
    depth1 = oracle_frame(dxrs, host, oracle, feature, False, 3, True, bounces=1)[1].rays - oracle_frame(dxrs, host, oracle, feature, False, 3, True, bounces=0)[1].rays
    assert depth1 > 3 * 64


# ------------------------------------------------------------------------------------------------------------------------- the forms
@pytest.fixture(scope="module")
def contexts(dxrs):
    """form -> its context, made on first use, profiling on; all closed at the end of the module"""
    made = {}

    def get(form):
        if form not in made:
            assert not any(k in os.environ for k in KNOBS)  # (the defaults are part of what is under test)
            env, flags = FORMS[form][:2]
            made[form] = context_under(dxrs, env, flags=flags)
            made[form].set_profiling(True)
        return made[form]

    yield get
    for r in made.values():
        r.close()


def _load(r, sc):
    info = r.set_scene(sc["spheres"], sc["materials"], sc["sd"])
    r.set_textures(sc["textures"])
    return info


def _check_tree(r, info, form):
    tree = FORMS[form][2]
    assert bool(info.lds_resident) == (tree == "lds")
    assert (info.node_count < 32767) == (tree != "g32")
    if tree != "lds":  # the walk of a tree in global memory: 4-wide records unless PT_WIDE=0
        assert (r.download_wide() is None) == (FORMS[form][0].get("PT_WIDE") == "0")


def _check_launches(st, form, spp, di):
    sequence = FORMS[form][3]
    got = (st.traverse_launches, st.shade_launches, st.tail_launches)
    if sequence == "polled":  # passes until the polled queue size drops below the threshold: at least the lag's two, then the looping pass
        assert st.traverse_launches >= 3 and st.shade_launches == 0 and st.tail_launches == 1, got
    else:
        assert got == expected_launches(sequence, spp, di), (form, spp, got)
    assert st.beams_used == (0 if sequence == "split" else 1)


def _cases(form):
    spps = FORMS[form][4]
    return [(spp, True) for spp in spps] + [(spps[0], False)]


@gpu
@pytest.mark.parametrize("feature", FEATURES[:-1])
@pytest.mark.parametrize("form", list(FORMS))
def test_form_renders_feature(dxrs, host, oracle, contexts, form, feature):
    big = FORMS[form][2] == "g32"
    sc = scene_of(dxrs, host, feature, big)
    r = contexts(form)
    try:
        _check_tree(r, _load(r, sc), form)
        r.set_camera(_camera(host, sc))
        for spp, rr in _cases(form):
            r.set_constants(_settings(dxrs, sc, spp, rr))
            r.profile(reset=True)  # (the pool of per-launch events starts over)
            img, st = render_rested(r)
            ref, ost = oracle_frame(dxrs, host, oracle, feature, big, spp, rr)
            print(f"{form} x {feature} spp {spp} rr {rr}: rays {st.rays} (oracle {ost.rays}), launches {st.traverse_launches}/{st.shade_launches}/{st.tail_launches}, "
                  f"beams {st.beams_used}, mismatches {count_mismatch(img, ref)}")
            assert count_mismatch(img, ref) == 0
            assert st.rays == ost.rays and st.paths == ost.paths
            assert np.isfinite(img).all()
            _check_launches(st, form, spp, sc["di"])
    finally:
        r.set_textures(None)


def _denoiser_rested(r, mode, w, h):
    """render_rested for pt_render_denoiser: three frames of the view -> (out, outputs, stats) of the third, which must equal the first"""
    import torch
    from dxrs_amd.abi_types import DENOISER_OUTPUTS
    dev = torch.device("cuda", 0)
    frames = []
    for _ in range(3):
        out = torch.from_numpy(np.full((h, w, 4), -7.0, dtype=np.float32)).to(dev)
        bufs = {name: torch.from_numpy(np.full((h, w, width), -7.0, dtype=np.float32)).to(dev) for name, width in DENOISER_OUTPUTS[mode]}
        torch.cuda.synchronize(dev)
        st = r.render_denoiser_device(mode, out.data_ptr(), {name: b.data_ptr() for name, b in bufs.items()}, want_stats=True)
        r.synchronize()
        frames.append((out.cpu().numpy(), {name: b.cpu().numpy() for name, b in bufs.items()}, st))
    (out0, bufs0, st0), (out, bufs, st) = frames[0], frames[2]
    assert st.rays == st0.rays and np.array_equal(bits(out), bits(out0))
    for name in bufs:
        assert np.array_equal(bits(bufs[name]), bits(bufs0[name])), name
    return out, bufs, st


_denoiser_base = {}


@gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_form_renders_denoiser_outputs(dxrs, host, oracle, contexts, form):
    """pt_render_denoiser over the scene with every material map, in the DLSS-RR mode (out = the radiance: against the oracle) and one NRD
    mode (out = the primary surface's radiance).  Every other output, and the NRD out, must equal bit for bit what the default context writes
    for the same spheres (fused, tree in LDS; for the 32 800 spheres of the 32-bit forms what a caller gets by default, the split schedule);
    the default context's own outputs are pinned to the oracle by test_denoiser_outputs.py."""
    big = FORMS[form][2] == "g32"
    sc = scene_of(dxrs, host, "denoiser", big)
    w, h = sc["w"], sc["h"]
    cam = _camera(host, sc)
    todo = [r for r in (contexts("fused"), contexts(form))]
    try:
        for spp, rr in _cases(form):
            gs = _settings(dxrs, sc, spp, rr)
            ref, ost = oracle_frame(dxrs, host, oracle, "denoiser", big, spp, rr)
            for mode in (DLSS_RR, REBLUR):
                key = (big, spp, rr, mode)
                if key not in _denoiser_base:  # the default context's outputs: made once, kept unchanged
                    base = todo[0]
                    _load(base, sc)
                    base.set_camera(cam)
                    base.set_constants(gs)
                    _denoiser_base[key] = _denoiser_rested(base, mode, w, h)[:2]
                want_out, want_bufs = _denoiser_base[key]
                r = todo[1]
                _check_tree(r, _load(r, sc), form)
                r.set_camera(cam)
                r.set_constants(gs)
                r.profile(reset=True)
                out, bufs, st = _denoiser_rested(r, mode, w, h)
                assert st.rays == ost.rays and st.paths == ost.paths
                if mode == DLSS_RR:
                    assert count_mismatch(out, ref) == 0
                    assert np.isfinite(out).all()
                assert np.array_equal(bits(out), bits(want_out)), mode
                assert sorted(bufs) == sorted(want_bufs)
                for name in bufs:
                    assert np.array_equal(bits(bufs[name]), bits(want_bufs[name])), (mode, name)
                _check_launches(st, form, spp, False)
    finally:
        for r in todo:
            r.set_textures(None)
