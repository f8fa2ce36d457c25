"""Skinned meshes (rz_skin_create, rz_skin_pose, rz_skin_destroy): the C-ABI structs and symbols, the kernel's register budget,
and the host partner rzh_skin_triangles against the numpy restatement of the specification (skin_ref.py), byte for byte --
everything that can be checked without a GPU."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import skin_ref as K
from rayzen_amd import _lib
from rayzen_amd import scene as S
from test_rays_abi import _kernel_metadata

MESHES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "meshes")


def test_skin_structs_and_symbols():
    L = _lib.hip()
    assert L.rz_sizeof(_lib.SIZEOF_SKIN_TRIANGLE) == 64 == C.sizeof(_lib.SkinTriangle) == S.SKIN_TRIANGLE.itemsize
    assert L.rz_sizeof(_lib.SIZEOF_MORPH_TRIANGLE) == 48 == C.sizeof(_lib.MorphTriangle) == S.MORPH_TRIANGLE.itemsize
    assert L.rz_sizeof(13) == 0 and L.rz_sizeof(16) == 0 and L.rz_sizeof(19) == 0     # unassigned: what other tests probe
    want = {"bones": 0, "pad": 12, "weights": 16}
    assert [f for f, _ in _lib.SkinTriangle._fields_] == list(want)
    for f, off in want.items():
        assert getattr(_lib.SkinTriangle, f).offset == off == S.SKIN_TRIANGLE.fields[f][1], f
    assert _lib.MorphTriangle.d.offset == 0 == S.MORPH_TRIANGLE.fields["d"][1]
    assert S.SKIN_TRIANGLE["weights"].shape == (3, 4) and S.MORPH_TRIANGLE["d"].shape == (3, 4)
    assert _lib.SKIN_DEVICE_ARGS == 1
    assert L.rz_abi_version() == _lib.ABI_VERSION == 5       # additive: the revision stays
    lib, host = C.CDLL(_lib.HIP_SO), C.CDLL(_lib.HOST_SO)
    for name in ("rz_skin_create", "rz_skin_pose", "rz_skin_destroy", "rz_skin_last_kernel_ms"):
        assert hasattr(lib, name) and name in _lib.HIP_SYMBOLS, name
    assert hasattr(host, "rzh_skin_triangles") and "rzh_skin_triangles" in _lib.HOST_SYMBOLS


def test_the_header_states_the_structs_as_the_library_compiled_them():
    """The field order of the two structs in include/rayzen_hip.h is what _lib mirrors (sizes come from rz_sizeof above)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "rayzen_hip.h")).read()
    skin = text[text.index("typedef struct rz_skin_triangle"):text.index("} rz_skin_triangle;")]
    assert skin.index("uint32_t bones[3];") < skin.index("uint32_t pad;") < skin.index("float    weights[3][4];")
    morph = text[text.index("typedef struct rz_morph_triangle"):text.index("} rz_morph_triangle;")]
    assert "float d[3][4];" in morph
    assert "#define RZ_SKIN_DEVICE_ARGS 1u" in text and "#define RZ_ABI_VERSION 5" in text


def test_skin_kernel_uses_no_scratch():
    meta = _kernel_metadata(_lib.HIP_SO)
    found = {k: v for k, v in meta.items() if "rz_skin_tris" in k}
    assert len(found) == 3, sorted(meta)         # skin + morphs, skin only, morphs only
    for name, (spill, priv) in found.items():
        assert spill == 0 and priv == 0, f"{name}: {spill} VGPRs spilled, {priv} B of scratch"


def test_pack_bones():
    assert S.pack_bones([[1, 2, 3, 255]]).tolist() == [1 | 2 << 8 | 3 << 16 | 255 << 24]


@functools.lru_cache(maxsize=None)
def _mesh(name):
    if name == "one":
        return S.make_cube(2)[5:6].copy()
    if name == "cube":
        return S.make_cube(1)
    if name == "monkey":
        return S.load_obj(os.path.join(MESHES, "monkey.obj"), 1)
    return S.make_blob(24, 2.8, 0)


def _host(rig):
    return S.skin_triangles(rig.rest, rig.skin, rig.bones, rig.morphs, rig.morph_weights)


@pytest.mark.parametrize("name,count", [("one", 1), ("cube", 12), ("monkey", 968), ("blob24", 6912)])
def test_host_partner_equals_the_restatement_on_every_generator(name, count):
    mesh = _mesh(name)
    assert len(mesh) == count
    names = []
    for rig in K.rigs(mesh):
        want, got = rig.pose(), _host(rig)
        assert got.tobytes() == want.tobytes(), f"{name}/{rig.name}"
        # pads and materialIndex are the rest triangle's, and something moved
        for f in ("pad0", "pad1", "pad2", "materialIndex", "tail_pad"):
            assert got[f].tobytes() == rig.rest[f].tobytes(), f"{name}/{rig.name}: {f}"
        moved = any(got[f].tobytes() != rig.rest[f].tobytes() for f in K.CORNERS)
        assert moved, f"{name}/{rig.name}: nothing moved"
        names.append(rig.name)
    assert names == ["bend", "random1", "random2", "random7", "random256", "wild_weights", "odd_rest", "morph1", "morph3",
                     "skin7_morph1", "skin256_morph3"]


def test_the_generators_cover_what_they_claim():
    mesh = _mesh("monkey")
    by_name = {r.name: r for r in K.rigs(mesh)}
    for nb in (1, 2, 7, 256):
        r = by_name[f"random{nb}"]
        assert r.n_bones == nb
        kept = r.skin["weights"] != 0
        assert sorted(set(kept.sum(axis=2).reshape(-1).tolist())) == [0, 1, 2, 3, 4]
        slots = (r.skin["bones"][:, :, None] >> (8 * np.arange(4, dtype=np.uint32))) & 255
        assert (slots[~kept] == 255).all() and (slots[kept] < nb).all()      # a skipped slot names bone 255
        assert np.signbit(r.skin["weights"][~kept]).any()                    # ... some with weight -0.0
        assert np.abs(r.bones.reshape(-1, 4, 4)[:, 3, :3]).max() > 100       # translations towards 1e3
    wild = by_name["wild_weights"].skin["weights"]
    assert (wild < 0).any() and (np.abs(wild.sum(axis=2) - 1) > 0.5).any()
    odd = by_name["odd_rest"].rest
    flat = np.concatenate([odd[f].reshape(-1) for f in K.CORNERS])
    assert (np.signbit(flat) & (flat == 0)).any() and ((flat != 0) & (np.abs(flat) < np.finfo(np.float32).tiny)).any()
    assert by_name["morph1"].skin is None and by_name["morph1"].n_morphs == 1 and by_name["morph3"].n_morphs == 3
    assert 0.0 in by_name["morph3"].morph_weights.tolist()
    d = by_name["morph3"].morphs["d"]
    assert (np.signbit(d) & (d == 0)).any()
    bend = by_name["bend"].skin["weights"]
    assert (bend[:, :, 0] == 0).any() and (bend[:, :, 1] == 0).any()         # the ends of the bend keep one influence


def test_a_corner_without_a_kept_influence_is_the_morphed_rest():
    rest = K.odd_rest(_mesh("cube"))
    rng = np.random.default_rng(3)
    skin = np.zeros(12, S.SKIN_TRIANGLE)
    skin["bones"] = S.pack_bones(np.full((12, 3, 4), 255))
    skin["weights"][:, :, 1] = np.float32(-0.0)
    bones = K.random_bones(rng, 3)
    morphs = K.random_morphs(rng, rest, 2)
    weights = np.array([0.5, -2.0], np.float32)
    got = S.skin_triangles(rest, skin, bones, morphs, weights)
    assert got.tobytes() == S.skin_triangles(rest, None, None, morphs, weights).tobytes() == K.pose(rest, None, None, morphs, weights).tobytes()
    assert got.tobytes() != rest.tobytes()
    # ... and without morphs: the rest bits themselves, signs of zero and denormals included
    assert S.skin_triangles(rest, skin, bones).tobytes() == rest.tobytes() == K.pose(rest, skin, bones).tobytes()
    # one kept influence with the identity and weight 1 is NOT a copy: w * q rounds -0.0 + 0 to +0.0 where the rest holds -0.0
    skin["weights"][:, :, 0] = 1.0
    skin["bones"] = 0
    one = S.skin_triangles(rest, skin, np.stack([S.identity()]))
    assert one.tobytes() == K.pose(rest, skin, np.stack([S.identity()])).tobytes()
    assert (one["v0"] == rest["v0"]).all()


def test_host_partner_refuses_what_the_device_refuses():
    L = _lib.host()
    rest = _mesh("cube")
    out = np.zeros(12, S.TRIANGLE)
    skin = np.zeros(12, S.SKIN_TRIANGLE)
    skin["weights"][:, :, 0] = 1.0
    skin["bones"][7, 2] = 2                       # bone 2 of a 2-bone rig, kept
    bones = np.stack([S.identity(), S.identity()])
    call = lambda sk, nb, mo, mw, nm: L.rzh_skin_triangles(rest.ctypes.data, sk, 12, bones.ctypes.data, nb, mo, mw, nm, out.ctypes.data)
    assert call(skin.ctypes.data, 2, None, None, 0) == -2
    assert (out.view(np.uint8) == 0).all()        # nothing written
    assert call(skin.ctypes.data, 0, None, None, 0) == -1
    assert call(skin.ctypes.data, 257, None, None, 0) == -1
    assert call(None, 2, None, None, 0) == -1
    assert call(None, 0, None, None, -1) == -1
    assert call(None, 0, None, None, 1) == -1
    skin["weights"][7, 2, 0] = 0.0                # the same slot skipped: its bone index is not looked at
    assert call(skin.ctypes.data, 2, None, None, 0) == 0
    with pytest.raises(RuntimeError):
        skin["weights"][7, 2, 0] = np.nan         # NaN does not compare equal to 0: kept
        S.skin_triangles(rest, skin, bones)
