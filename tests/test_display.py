"""The validation epoch's pictures and per-coil table, host side: a float64 numpy restatement of the three formulas
(save_im's k-space display, imsave's gray quantisation, stats_per_coil -- models/utils.py:254-287) checked against what the
reference itself produced (tests/golden/display.npz, written by tools/make_golden_display.py), the PNG writer / reader,
the closed form of matplotlib's 'gray' table, the --data_samples expansion and the table text.  No GPU."""
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN

U32 = 2.0 ** -24  # unit roundoff of fp32


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "display.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


# ---- float64 restatement -------------------------------------------------------------------------------------------
def kspace_display64(coils, minus=None, sf=8.0):
    """models/utils.py:262-267 in float64 on fp32 inputs: complex_abs, RSS over coils, * expm1(sf) / max, log1p, / max.
    The error picture's input is the fp32 difference the reference hands to save_im (train.py:225)."""
    z = coils if minus is None else (coils.astype(np.float32) - minus.astype(np.float32))
    z = z.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.sqrt((np.sqrt((z ** 2).sum(-1)) ** 2).sum(0))
        g = g * (np.expm1(np.float64(sf)) / g.max())
        g = np.log1p(g)
        return g / g.max()


def gray_norm64(img, take_abs=False, vmin=None, vmax=None):
    """n of imsave's Normalize in float64: (x - vmin) / (vmax - vmin), the picture's own extrema unless both bounds are
    given and non-zero (save_im's ``if vmin and vmax``); all zeros when vmax == vmin; NaN where x is not finite."""
    x = np.asarray(img, dtype=np.float64)
    if take_abs:
        x = np.abs(x)
    ok = np.isfinite(x)
    if not (vmin and vmax):
        vmin, vmax = (x[ok].min(), x[ok].max()) if ok.any() else (0.0, 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.zeros_like(x) if vmax == vmin else (x - vmin) / (vmax - vmin)
    return np.where(ok, n, np.nan)


def gray_index64(n):
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(n), 0, np.clip(np.floor(np.nan_to_num(n) * 256.0), 0, 255)).astype(np.int64)


def gray_bytes64(n, lut):
    """index min(floor(256 n), 255), 0 below, 255 above; byte lut[index]; masked (NaN) pixels are 0."""
    return np.where(np.isnan(n), 0, lut[gray_index64(n)]).astype(np.uint8)


def coil_stats64(coils):
    v = np.asarray(coils, dtype=np.float64).reshape(coils.shape[0], -1)
    return np.stack([v.mean(1), v.std(1, ddof=1), v.max(1), v.min(1)], axis=1)


def assert_bytes(got, n64, lut, tol, label=""):
    """The byte rule: a pixel may differ from the restatement only by exactly one index step, and only where 256 n lies
    within 256 * tol of an integer.  Returns the number of such pixels."""
    got = np.asarray(got)
    want = gray_bytes64(n64, lut)
    diff = got != want
    if not diff.any():
        return 0
    idx = gray_index64(n64)
    t = np.nan_to_num(n64) * 256.0
    near = np.abs(t - np.rint(t)) <= 256.0 * tol
    one_step = (got == lut[np.clip(idx + 1, 0, 255)]) | (got == lut[np.clip(idx - 1, 0, 255)])
    bad = diff & ~(near & one_step & ~np.isnan(n64))
    assert not bad.any(), (label, int(bad.sum()), got[bad][:5], want[bad][:5], t[bad][:5])
    return int(diff.sum())


# ---- the restatement against the reference's outputs ----------------------------------------------------------------
CASES = {  # tag -> (input key, minus key, is_kspace, take_abs, with range)
    "kspace_case": ("kspace", None, True, False, False),
    "error_case": ("second", "kspace", True, False, False),
    "image_case": ("image", None, False, True, False),
    "ranged_case": ("ranged", None, False, True, True),
    "constant_case": ("constant", None, False, True, False),
}


def case_n64(gold, tag):
    """(float64 display or None, float64 n) of a fixture case"""
    key, minus, is_kspace, take_abs, ranged = CASES[tag]
    disp = None
    if is_kspace:
        disp = kspace_display64(gold[key], None if minus is None else gold[minus], float(gold["smoothing_factor"]))
        return disp, gray_norm64(disp)
    lo, hi = (float(v) for v in gold["ranged_vmin_vmax"]) if ranged else (None, None)
    return disp, gray_norm64(gold[key], take_abs, lo, hi)


@pytest.mark.parametrize("tag", list(CASES))
def test_restatement_against_reference(gold, tag):
    C = gold["kspace"].shape[0]
    disp, n = case_n64(gold, tag)
    # fp32 evaluation of the chain against float64: (C / 2 + 2) u on the RSS, 4 u on the scale and the product, log1p
    # does not amplify a relative error (y / (1 + y) < 1) and its values reach sf = 8, the division by their maximum
    # brings them back to 0..1 -> about 2 (C / 2 + 8) u; 32 u covers C = 4.  Normalize adds three more roundings.
    tol = 32 * U32
    if disp is not None:
        d = float(np.abs(gold[tag + "/handed"].astype(np.float64) - disp).max())
        print(f"{tag}: max |reference fp32 - float64| of the display = {d:.3e} (bound {tol:.3e})")
        assert d <= tol
        assert abs(disp.max() - 1.0) < 1e-15 and disp.min() >= 0.0
    dn = float(np.nanmax(np.abs(gold[tag + "/normalized"].astype(np.float64) - n)))
    print(f"{tag}: max |matplotlib n - float64 n| = {dn:.3e}")
    assert dn <= tol + 8 * U32
    assert_bytes(gold[tag + "/bytes"], n, gold["lut"], tol + 8 * U32, tag)


def test_fixture_pins_the_corner_cases(gold):
    assert not gold["constant_case/bytes"].any()  # vmax == vmin: all zeros
    assert (gold["image"] < 0).any() and gold["image_case/bytes"].max() == 255
    b = gold["ranged_case/bytes"]
    lo, hi = gold["ranged_vmin_vmax"]
    assert (b[gold["ranged"] < lo] == 0).all() and (b[gold["ranged"] > hi] == 255).all()
    assert (gold["ranged"] < lo).any() and (gold["ranged"] > hi).any()
    mag = np.sqrt((gold["kspace"].astype(np.float64) ** 2).sum(-1))
    assert mag.max() / mag[mag > 0].min() > 1e4  # several decades, as a scan's k-space


def test_lut_closed_form_equals_matplotlibs_table(gold):
    from inr_mi355x.display import gray_lut
    lut = gray_lut()
    assert lut.dtype == np.uint8 and np.array_equal(lut, gold["lut"])
    assert not np.array_equal(lut, np.arange(256)) and lut[33] == 32 and lut[37] == 36 and lut[255] == 255


def test_coil_stats_restatement_and_table(gold):
    from inr_mi355x.display import STATS_TITLE, coil_stats_table
    k = gold["kspace"]
    want, ref = coil_stats64(k), gold["coil_stats"]  # ref: the reference's fp32 torch numbers
    n = k[0].size
    mean_abs = np.abs(k.astype(np.float64)).reshape(k.shape[0], -1).mean(1)
    # an fp32 sum of n terms is within n u sum|x| of the exact one; std inherits the relative form of that bound
    assert (np.abs(ref[:, 0] - want[:, 0]) <= n * U32 * mean_abs).all()
    assert (np.abs(ref[:, 1] - want[:, 1]) <= n * U32 * want[:, 1]).all()
    assert np.array_equal(ref[:, 2:], want[:, 2:])
    text = coil_stats_table(ref)
    lines = text.splitlines()
    assert lines[0] == STATS_TITLE == str(gold["coil_stats_text"]).splitlines()[0]
    assert lines[1].split() == ["coil", "mean", "std", "max", "min"]

    def numbers(t):
        return [[float(v) for v in row.split()] for row in t.splitlines()[3:] if row.strip()]
    got = np.array(numbers(text))
    assert got.shape == (k.shape[0], 5) and np.array_equal(got[:, 0], np.arange(k.shape[0]))
    np.testing.assert_allclose(got[:, 1:], ref, rtol=1e-5)  # six significant digits are printed
    np.testing.assert_allclose(got, np.array(numbers(str(gold["coil_stats_text"]))), rtol=1e-5)


# ---- PNG ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (7, 7), (24, 20), (64, 1000)])
def test_png_round_trip(tmp_path, shape):
    from inr_mi355x.display import read_png_gray, write_png_gray
    rng = np.random.RandomState(shape[0])
    a = rng.randint(0, 256, size=shape).astype(np.uint8)
    p = str(tmp_path / "a.png")
    write_png_gray(p, a)
    assert np.array_equal(read_png_gray(p), a)
    import torch
    write_png_gray(p, torch.from_numpy(a))
    assert np.array_equal(read_png_gray(p), a)


def test_png_is_read_by_pil_and_reader_reads_pils(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from inr_mi355x.display import read_png_gray, write_png_gray
    a = (np.arange(48 * 37) * 7 % 256).astype(np.uint8).reshape(48, 37)
    p = str(tmp_path / "a.png")
    write_png_gray(p, a)
    with Image.open(p) as im:
        assert im.mode == "L" and im.size == (37, 48)
        assert np.array_equal(np.asarray(im), a)
    q = str(tmp_path / "b.png")
    Image.fromarray(a).save(q, optimize=True)  # PIL picks scanline filters of its own
    assert np.array_equal(read_png_gray(q), a)


def test_png_rejects_what_it_does_not_write(tmp_path):
    from inr_mi355x.display import read_png_gray, write_png_gray
    with pytest.raises(ValueError, match="uint8"):
        write_png_gray(str(tmp_path / "x.png"), np.zeros((4, 4), dtype=np.float32))
    (tmp_path / "y.png").write_bytes(b"not a png")
    with pytest.raises(ValueError, match="not a PNG"):
        read_png_gray(str(tmp_path / "y.png"))


def test_prepare_sub_folder(tmp_path, capsys):
    from inr_mi355x.display import prepare_sub_folder
    ck, im = prepare_sub_folder(str(tmp_path / "out"))
    assert ck == str(tmp_path / "out" / "checkpoints") and im == str(tmp_path / "out" / "images")
    assert os.path.isdir(ck) and os.path.isdir(im)
    assert capsys.readouterr().out.count("Creating directory: ") == 2
    assert prepare_sub_folder(str(tmp_path / "out")) == (ck, im) and capsys.readouterr().out == ""


# ---- --data_samples -------------------------------------------------------------------------------------------------
def test_expand_data_samples(tmp_path):
    import yaml
    from inr_mi355x.train import expand_data_samples, get_config
    p = tmp_path / "samples.yaml"
    p.write_text(yaml.safe_dump({"samples": {3: [10, 12], 7: [0]}}))
    samples = get_config(str(p))["samples"]
    cfg = {"model": "SIREN", "sample": 0, "slice": 5, "net": {"network_width": 32}}
    fits = expand_data_samples(cfg, samples)
    assert [sub for _, sub in fits] == ["sample_3_slice_10", "sample_3_slice_12", "sample_7_slice_0"]
    assert [(c["sample"], c["slice"]) for c, _ in fits] == [(3, 10), (3, 12), (7, 0)]  # the sample comes from the loop
    assert all(c["model"] == "SIREN" and c["net"] == cfg["net"] for c, _ in fits)
    assert cfg["sample"] == 0 and cfg["slice"] == 5  # the caller's config is left alone
    for empty in (None, {}):
        one = expand_data_samples(cfg, empty)
        assert len(one) == 1 and one[0][0] is cfg and one[0][1] == ""


def test_display_wrappers_refuse_the_cpu():
    import torch
    from inr_mi355x import display as D
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.kspace_display(torch.zeros(2, 8, 8, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.gray8(torch.zeros(8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.coil_stats(torch.zeros(2, 8, 8, 2))
    with pytest.raises(RuntimeError, match=r"expected \[C,H,W,2\]"):
        D.coil_stats(torch.zeros(2, 8, 8))
