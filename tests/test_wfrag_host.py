"""The weight-fragment writers of csrc/dsphere_wfrag.h, run on the CPU (tools/wfrag_image.hip, compiled for the host alone) against the
numpy yardstick tests/wfrag_ref.py: every form, both operand geometries, the block-diagonal `pack` gather, zero padding -- bit for bit
-- and the facts the kernels rely on (what a split adds up to, the two rules for the third bf16x6 term)."""

import itertools
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import wfrag_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
pytestmark = pytest.mark.skipif(HIPCC is None, reason="no hipcc: the host program of tools/wfrag_image.hip cannot be built")

K = 3


def _f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def weight_values(form, n, seed):
    """n float32 values: the special ones first, random signs and mantissas over the form's magnitudes behind them"""
    rng = np.random.default_rng(seed)
    if form == ref.F16X3:  # the scaled range of an f16 image: the caller puts the largest weight in [2048, 4096)
        special = np.array([0.0, -0.0, 2.0**-12, -(2.0**-12), 4095.75, -4095.75, 2048.0, 1.0, -1.0, 1.0 + 2.0**-11, 1.0 + 3 * 2.0**-11,
                            -(1.0 + 2.0**-11), 3.0009765625], dtype=np.float32)  # (1 + 2^-11, 1 + 3 2^-11: f16 ties under an even and an odd hi)
        mag = np.exp2(rng.uniform(-12, 12, n)) * rng.choice([-1.0, 1.0], n)
        vals = np.clip(np.abs(mag), 2.0**-12, 4095.75) * np.sign(mag)
    else:
        special = np.concatenate([
            np.array([0.0, -0.0, 1.0, -1.0, 1.5, -0.0078125, 2.0**-30, -(2.0**-30), 2.0**30, -(2.0**30), 255.0 * 2.0**20], dtype=np.float32),  # exact bf16 values
            # round-to-even ties of the hi term: low 16 bits 0x8000 under an even (..80) and an odd (..81) upper half, both signs
            _f32([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x4B7E8000, 0x4B7F8000, 0x307F8000]),
            # .. and of the lo term: v - hi ends in a tie (hi = 1.0, remainder 2^-9 (1 + 2^-7 k + 2^-8))
            _f32([0x3F804080, 0x3F804180, 0xBF804080, 0xBF804180]),
            _f32([0x3F7FFFFF, 0x3F800001, 0x4E7FFFFF, 0xB0FFFFFF]),  # full mantissas
        ])
        vals = (1.0 + rng.random(n)) * np.exp2(rng.integers(-30, 30, n)) * rng.choice([-1.0, 1.0], n)
    out = np.concatenate([special, vals.astype(np.float32)])[:n].astype(np.float32)
    assert out.size == n
    return out


def make_cases():
    cases = []
    shapes = [(3, 5), (20, 40), (3, 40), (20, 5)]
    for (name, form), geometry, pack, (Fin, Fout) in itertools.product(ref.FORMS.items(), (32, 16), (0, 2, 4), shapes):
        if pack and geometry != 32:
            continue  # the block diagonal is the tile kernels': 32x32 operands
        slice_len = 16 if geometry == 32 else 32  # (and `geometry` columns per block)
        slices, blocks = (1, 2) if pack else ((Fin + slice_len - 1) // slice_len, (Fout + geometry - 1) // geometry)
        ld = Fout + 3  # (a leading dimension that is not the width)
        seed = len(cases)
        w = weight_values(form, Fin * K * ld, seed).reshape(Fin * K, ld)
        np.random.default_rng(seed).shuffle(w.reshape(-1))  # the special values anywhere, padding included
        scale = 1.0 if pack else (-2.0 if seed % 3 == 0 else (0.5 if seed % 3 == 1 else 1.0))  # (powers of two: an f16 image's range holds)
        if form == ref.F16X3 and not pack:
            scale = -1.0 if seed % 2 else 1.0
        cases.append(dict(id=f"{name}-g{geometry}-pack{pack}-{Fin}x{Fout}", form=form, geometry=geometry, pack=pack, Fin=Fin, Fout=Fout, k=seed % K,
                          ld=ld, slices=slices, blocks=blocks, scale=scale, w=w))
    return cases


CASES = make_cases()
# below 2^-110 the third bf16x6 term's two rules part: v = 2^-120 (1 + 2^-13 + 2^-14 + 2^-15) leaves 2^-134 + 2^-135 behind hi = 2^-120 and
# mid = 2^-133, under the last place of a subnormal bf16 (2^-133): truncation gives 0, rounding to nearest 2^-133
TINY = np.float32(2.0**-120 * (1 + 2.0**-13 + 2.0**-14 + 2.0**-15))
TINY_CASE = dict(id="bf16x6-subnormal-third-term", form=ref.BF16X6, geometry=32, pack=0, Fin=1, Fout=1, k=0, ld=1, slices=1, blocks=1, scale=1.0,
                 w=np.full((1, 1), TINY, dtype=np.float32))


def record(c):
    head = struct.pack("<12i", c["geometry"], c["form"], c["Fin"], c["Fout"], K if c is not TINY_CASE else 1, c["k"], c["ld"], c["pack"], c["slices"],
                       c["blocks"], c["w"].shape[0], 0)
    return head + struct.pack("<f", c["scale"]) + np.ascontiguousarray(c["w"], dtype=np.float32).tobytes()


@pytest.fixture(scope="module")
def images(tmp_path_factory):
    """one build of the host program and one run of it over every case: {case id: image bytes as uint8}"""
    d = tmp_path_factory.mktemp("wfrag")
    exe = str(d / "wfrag_image")
    r = subprocess.run([HIPCC, "--offload-host-only", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I",
                        os.path.join(ROOT, "deepsphere-cosmo-tf2_amd", "csrc"), os.path.join(ROOT, "tools", "wfrag_image.hip"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    allc = CASES + [TINY_CASE]
    (d / "cases.bin").write_bytes(b"".join(record(c) for c in allc))
    r = subprocess.run([exe, str(d / "cases.bin"), str(d / "images.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    blob = np.fromfile(str(d / "images.bin"), dtype=np.uint8)
    out, at = {}, 0
    for c in allc:
        n = c["slices"] * c["blocks"] * ref.group_bytes(c["form"])
        out[c["id"]] = blob[at:at + n]
        at += n
    assert at == blob.size
    return out


def yardstick(c):
    return ref.image(c["w"], c["geometry"], c["form"], c["Fin"], c["Fout"], K, c["k"], c["pack"], c["slices"], c["blocks"], c["scale"])


def test_cases_cover_what_they_should():
    ids = [c["id"] for c in CASES]
    assert len(set(ids)) == len(ids)
    for name in ref.FORMS:
        for g in (32, 16):
            assert any(i.startswith(f"{name}-g{g}-pack0") for i in ids)
        for p in (2, 4):
            assert any(i.startswith(f"{name}-g32-pack{p}") for i in ids)
    v = weight_values(ref.BF16X3, 4096, 0)
    bits = ref.f32_bits(v)
    tie = (bits & 0xFFFF) == 0x8000
    assert (tie & ((bits >> 16) & 1 == 0)).any() and (tie & ((bits >> 16) & 1 == 1)).any()
    assert (np.signbit(v) & (v == 0)).any() and (~np.signbit(v) & (v == 0)).any()
    assert np.abs(v[v != 0]).min() <= 2.0**-29 and np.abs(v).max() >= 2.0**29
    assert ((bits & 0xFFFF) == 0).sum() >= 8  # exact bf16 values
    f = np.abs(weight_values(ref.F16X3, 4096, 0))
    assert f[f != 0].min() == 2.0**-12 and f.max() < 4096 and f.max() > 2048


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_image_is_the_yardsticks_bit_for_bit(images, case):
    got, want = images[case["id"]], yardstick(case)
    assert got.size == want.size
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} bytes differ, the first at {bad[0]}: {got[bad[0]]:#x} for {want[bad[0]]:#x}"
    # padding is zero: every (lane, slot) past the layer's channels or columns holds +0 in every term
    for g in range(case["slices"] * case["blocks"]):
        c_, nb = divmod(g, case["blocks"])
        v = ref.gather(case["w"], case["geometry"], c_, nb, case["Fin"], case["Fout"], K, case["k"], case["pack"], case["scale"])
        inside = ref.gather(np.ones_like(case["w"]), case["geometry"], c_, nb, case["Fin"], case["Fout"], K, case["k"], case["pack"], 1.0) != 0
        grp = got[g * ref.group_bytes(case["form"]):(g + 1) * ref.group_bytes(case["form"])]
        for term in ref.values(grp, case["form"]):
            assert not np.any(ref.f32_bits(term)[~inside]), "a padded element is not +0"
        # what the kernels rely on, from the program's own image
        terms = ref.values(grp, case["form"])
        if case["form"] == ref.BF16X6:
            assert np.array_equal(ref.f32_bits((terms[0] + terms[1]) + terms[2])[v != 0], ref.f32_bits(v)[v != 0]), "hi + mid + lo != v in float32"
            assert np.array_equal(((terms[0] + terms[1]) + terms[2]) == 0, v == 0)
        elif case["form"] == ref.BF16X3:
            # an 8-bit round to nearest is within 2^-8 |x| of x: |v - hi| <= 2^-8 |v|, |(v - hi) - lo| <= 2^-16 |v|
            err = np.abs(v.astype(np.float64) - (terms[0].astype(np.float64) + terms[1].astype(np.float64)))
            assert np.all(err <= 2.0**-16 * np.abs(v.astype(np.float64)))
        elif case["form"] == ref.F16X3:
            # 11 + 11 bits: within 2^-22 |v|, or within half the spacing of the subnormal f16 (2^-25) where lo has left the normal range
            err = np.abs(v.astype(np.float64) - (terms[0].astype(np.float64) + terms[1].astype(np.float64)))
            assert np.all(err <= np.maximum(2.0**-22 * np.abs(v.astype(np.float64)), 2.0**-25))
        else:
            assert np.array_equal(ref.f32_bits(terms[0]), ref.f32_bits(v))


def test_third_bf16x6_term_truncated_and_rounded_agree_on_normal_remainders():
    """every value the bf16x6 cases use (|v| >= 2^-30, far above 2^-110): the remainder has at most eight significant bits, so both rules
    give the same 16 bits"""
    n = 0
    for c in CASES:
        if c["form"] != ref.BF16X6:
            continue
        v = (np.float32(c["scale"]) * c["w"]).reshape(-1)
        assert np.array_equal(ref.split_bf16x6(v, "rne")[2], ref.split_bf16x6(v, "trunc")[2])
        n += v.size
    assert n > 1000


def test_third_bf16x6_term_below_the_stated_magnitude_follows_the_headers_rule(images):
    """|v| < 2^-110: the rules may part (here they do), and the header's is the rounding convert"""
    hi, mid, lo_rne = ref.split_bf16x6(np.array([TINY]), "rne")
    lo_trunc = ref.split_bf16x6(np.array([TINY]), "trunc")[2]
    assert (hi[0], mid[0], lo_rne[0], lo_trunc[0]) == (0x0380, 0x0001, 0x0001, 0x0000)
    img = images[TINY_CASE["id"]].view(np.uint16)
    assert (img[0], img[512], img[1024]) == (hi[0], mid[0], lo_rne[0])
