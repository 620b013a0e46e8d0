"""The hyperparameter search (inr_mi355x/hp_search.py) on the MI355X: every trial's statistics against a standalone
INRTrainer fit of the same merged config (bit-equal: same kernels, same data, same seeds), the seeding order of
hp_model_training.py:46-49 against the reference's initial weights (tests/golden/hp_search.json), one ingest per distinct
dataset with clean data for the next trial, worker processes against the in-process search, recorded refusals, and the
command line with its pictures.  Synthetic make_kspace(4, 64, 48), SIREN 3 x 64 behind a gauss encoder of size 32,
batches of 1024 rows, two epochs with a validation after each.  Every child process runs under a timeout."""
import copy
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch
import yaml

from conftest import GOLDEN, PKG, ROOT

pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(GOLDEN, "hp_search.json")))
BASE = dict(GOLD["base_config"], log_iter=1000)
SHAPE = (4, 64, 48)
MAX_EPOCH = 2
STATS = ("best_psnr", "best_psnr_ep", "best_ssim", "best_ssim_ep")
TIMING = ("fit_seconds", "setup_seconds", "worker")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def grid_hp(**space):
    return {"method": "grid", "max_epoch": MAX_EPOCH,
            "search_space": {k: {"values": v, "type": "item"} for k, v in space.items()}}


def standalone(merged, dev):
    """The four statistics of a plain INRTrainer fit of ``merged``: fresh data, every batch of every epoch, validate()
    after each epoch."""
    from inr_mi355x import hp_search as HS
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train import INRTrainer
    cfg = HS.trial_config(merged, MAX_EPOCH)
    image, coords, shape = make_kspace(*SHAPE, normalization=cfg["normalization"], image_space=bool(cfg["transform"]))
    tr = INRTrainer(cfg, image, coords, shape, dev, seed=0, model_seed=42)
    for epoch in range(MAX_EPOCH):
        for it in range(tr.steps_per_epoch):
            tr.step(epoch, it)
        tr.validate(epoch)
    return {"best_psnr": tr.best_psnr, "best_psnr_ep": tr.best_psnr_ep, "best_ssim": tr.best_ssim,
            "best_ssim_ep": tr.best_ssim_ep}, tr.global_step


def assert_trials_equal_standalone(res, dev):
    from inr_mi355x import hp_search as HS
    hps = [r["hp"] for r in res["results"]]
    merged = HS.merged_configs(BASE, hps)
    want = []
    for r, m in zip(res["results"], merged):
        w, steps = standalone(m, dev)
        got = {k: r[k] for k in STATS}
        print("trial {} {}: search {} standalone {}".format(r["index"], r["hp"], got, w))
        assert got == w and r["steps"] == steps == MAX_EPOCH * 12, (r, w)  # 4*64*48 rows / 1024
        assert r["best_psnr"] > 0 and 0 < r["best_ssim"] <= 1
        want.append(w)
    return merged, want


def first_argmax(values):
    return max(range(len(values)), key=lambda i: (values[i], -i))


def test_grid_trials_equal_standalone_fits(dev, tmp_path):
    from inr_mi355x import hp_search as HS
    from inr_mi355x.train import set_default_configs
    res = HS.run_search(BASE, grid_hp(**{"lr": [1e-4, 1e-3], "encoder.scale": [2, 4]}), str(tmp_path), synthetic=SHAPE)
    assert [r["hp"] for r in res["results"]] == [{"lr": 1e-4, "encoder.scale": 2}, {"lr": 1e-4, "encoder.scale": 4},
                                                 {"lr": 1e-3, "encoder.scale": 2}, {"lr": 1e-3, "encoder.scale": 4}]
    assert not res["aborted"] and res["ingests"] == 1
    merged, want = assert_trials_equal_standalone(res, dev)
    assert len({w["best_psnr"] for w in want}) == 4  # the four trials are four different fits
    for m, name in (("psnr", "best_psnr_config.yaml"), ("ssim", "best_ssim_config.yaml")):
        i = first_argmax([w["best_" + m] for w in want])
        assert res["best_" + m]["index"] == i + 1 and res["best_" + m]["value"] == want[i]["best_" + m]
        # (the file holds the config the search ran: the reference's defaults filled in, hp_search_script.py:79)
        assert yaml.safe_load(open(tmp_path / name)) == set_default_configs(copy.deepcopy(merged[i]))
    assert all(r["fit_seconds"] > 0 and r["setup_seconds"] > 0 and r["worker"] == 0 for r in res["results"])


def _hashes(sd):
    out = {}
    for k, v in sd.items():
        v = v.detach().cpu()
        out[k] = hashlib.sha256((torch.view_as_real(v) if v.is_complex() else v).contiguous().numpy().tobytes()).hexdigest()
    return out


def test_model_seed_42_gives_the_references_initial_weights(dev):
    """hp_model_training.py:46-49: the encoder is drawn first (here from ``seed``), then torch.manual_seed(42), then the
    model.  model_seed=None with seed=42 gives the same weights only where the encoder draws nothing before the model:
    WIRE on raw coordinates (embedding 'none') -- not the SIREN behind a gauss encoder, whose matrix B takes the first
    draws of the stream."""
    from inr_mi355x import hp_search as HS
    from inr_mi355x.synthetic import make_kspace
    from inr_mi355x.train import INRTrainer
    data = make_kspace(*SHAPE)
    siren = HS.trial_config(BASE, MAX_EPOCH)
    assert siren["net"] == GOLD["init"]["SIREN"]["net"]
    tr = HS.build_trial_trainer(siren, data, seed=0, device=dev)
    assert _hashes(tr.model.state_dict()) == GOLD["init"]["SIREN"]["sha256"]
    other_B = HS.build_trial_trainer(siren, data, seed=5, device=dev)
    assert _hashes(other_B.model.state_dict()) == GOLD["init"]["SIREN"]["sha256"]
    assert not torch.equal(other_B.encoder.B, tr.encoder.B)  # --seed moves the encoder alone
    plain = INRTrainer(siren, *data, dev, seed=42)
    assert _hashes(plain.model.state_dict()) != GOLD["init"]["SIREN"]["sha256"]
    wire = dict(siren, model="WIRE", net=GOLD["init"]["WIRE"]["net"],
                encoder=dict(embedding="none", scale=0, embedding_size=0, coordinates_size=3))
    assert _hashes(HS.build_trial_trainer(wire, data, seed=0, device=dev).model.state_dict()) == GOLD["init"]["WIRE"]["sha256"]
    assert _hashes(INRTrainer(wire, *data, dev, seed=42).model.state_dict()) == GOLD["init"]["WIRE"]["sha256"]
    # and None is today's trainer, bit for bit
    a, b = INRTrainer(siren, *data, dev, seed=3), INRTrainer(siren, *data, dev, seed=3, model_seed=None)
    assert _hashes(a.model.state_dict()) == _hashes(b.model.state_dict()) and torch.equal(a.encoder.B, b.encoder.B)


def test_normalization_as_item_key_one_ingest_per_value_and_clean_data(dev, tmp_path):
    from inr_mi355x import hp_search as HS
    hp = {"method": "random", "max_epoch": MAX_EPOCH, "num_search": 5,
          "search_space": {"normalization": {"values": ["coil", "max"], "type": "item"},
                           "lr": {"values": [1e-4, 1e-3], "type": "log"}}}
    res = HS.run_search(BASE, hp, str(tmp_path), synthetic=SHAPE, search_seed=2)
    norms = [r["hp"]["normalization"] for r in res["results"]]
    print("sampled normalisations:", norms)
    assert len(set(norms)) == 2 and any(a != b for a, b in zip(norms, norms[1:]))  # a trial follows the other scheme
    assert res["ingests"] == len(set(norms)) == 2
    assert_trials_equal_standalone(res, dev)
    again = HS.run_search(BASE, hp, str(tmp_path), synthetic=SHAPE, search_seed=2, cache_bytes=0)
    assert again["ingests"] == 5
    assert [{k: r[k] for k in STATS} for r in again["results"]] == [{k: r[k] for k in STATS} for r in res["results"]]


def test_trials_leave_the_cached_tensors_alone(dev):
    from inr_mi355x import hp_search as HS
    runner = HS.LocalRunner(HS.synthetic_source(*SHAPE), MAX_EPOCH, seed=0, device=dev, extra_key=SHAPE)
    image, coords, shape = runner.cache.get(BASE)
    assert image.device.type == "cuda" and coords.device.type == "cuda" and shape == SHAPE
    keep = image.clone(), coords.clone()
    first = runner(dict(BASE, config_index=1))
    for extra in (dict(shuffle=True), dict(undersampling="grid-2*2"), dict(per_coil=True, batch_size=1)):
        cfg = dict(copy.deepcopy(BASE), config_index=2, **extra)
        res = runner(cfg)
        assert "error" not in res, res
        key_image, key_coords, _ = runner.cache.get(cfg)
        if set(extra) <= {"shuffle"}:
            assert key_image is image
    assert torch.equal(image, keep[0]) and torch.equal(coords, keep[1])
    last = runner(dict(BASE, config_index=3))
    assert {k: last[k] for k in STATS} == {k: first[k] for k in STATS}


def test_two_workers_equal_one_process(dev, tmp_path):
    from inr_mi355x import hp_search as HS
    hp = grid_hp(**{"lr": [1e-4, 3e-4, 1e-3], "normalization": ["coil", "max"]})
    for sub in ("one", "two"):
        os.makedirs(tmp_path / sub)
    one = HS.run_search(BASE, hp, str(tmp_path / "one"), synthetic=SHAPE)
    two = HS.run_search(BASE, hp, str(tmp_path / "two"), synthetic=SHAPE, jobs=2, trial_timeout=300)
    assert not two["aborted"], two["reason"]

    def untimed(rows):
        return [{k: v for k, v in r.items() if k not in TIMING} for r in rows]

    assert untimed(two["results"]) == untimed(one["results"]) and len(two["results"]) == 6
    assert {r["worker"] for r in two["results"]} <= {0, 1}
    on_disk = json.load(open(tmp_path / "two" / "results.json"))
    assert on_disk["aborted"] is False and [r["index"] for r in on_disk["results"]] == [1, 2, 3, 4, 5, 6]
    assert untimed(on_disk["results"]) == untimed(one["results"])
    for name in ("best_psnr_config.yaml", "best_ssim_config.yaml", "configs_and_results.txt"):
        assert open(tmp_path / "two" / name).read() == open(tmp_path / "one" / name).read()


def _run_cli(args, timeout=600):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT]))
    return subprocess.run([sys.executable, "-m", "inr_mi355x.hp_search"] + [str(a) for a in args], cwd=PKG, env=env,
                          capture_output=True, text=True, timeout=timeout)


def _write(tmp_path, hp):
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(yaml.safe_dump(BASE))
    hpf = tmp_path / "hp.json"
    hpf.write_text(json.dumps(hp))
    return cfg, hpf


def test_a_refused_value_is_recorded_and_the_search_goes_on(dev, tmp_path):
    cfg, hpf = _write(tmp_path, grid_hp(**{"net.network_width": [64, 1024], "lr": [1e-4, 1e-3]}))
    r = _run_cli(["--config", cfg, "--hp_config", hpf, "--output_path", tmp_path, "--synthetic", "4,64,48"])
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    rows = json.load(open(os.path.join(line["output_directory"], "results.json")))["results"]
    assert [x["hp"]["net.network_width"] for x in rows] == [64, 64, 1024, 1024]
    assert all(set(STATS) <= set(x) for x in rows[:2])
    for x in rows[2:]:
        assert "widths 1..512" in x["error"] and not set(STATS) & set(x), x
    assert not line["aborted"] and line["best_psnr"]["index"] in (1, 2) and line["best_ssim"]["index"] in (1, 2)
    best = yaml.safe_load(open(os.path.join(line["output_directory"], "best_psnr_config.yaml")))
    assert best["net"]["network_width"] == 64  # the winner's config, not the last trial's
    assert len(open(os.path.join(line["output_directory"], "configs_and_results.txt")).read().splitlines()) == 4


def test_cli_end_to_end_with_pictures(dev, tmp_path):
    from inr_mi355x import display as D
    hp = {"method": "random", "max_epoch": MAX_EPOCH, "num_search": 3,
          "search_space": {"lr": {"values": [1e-4, 1e-3], "type": "log"},
                           "net.network_depth": {"values": [2, 3], "type": "int"}}}
    cfg, hpf = _write(tmp_path, hp)
    args = ["--config", cfg, "--hp_config", hpf, "--output_path", tmp_path, "--synthetic", "4,64,48", "--save-images",
            "--search-seed", 5, "--jobs", 2, "--trial-timeout", 300]
    r = _run_cli(args)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "** Running Random Search **" in r.stdout
    line = json.loads(r.stdout.strip().splitlines()[-1])
    out = line["output_directory"]
    assert os.path.relpath(out, tmp_path).startswith(os.path.join("outputs", "cfg", "synthetic", "img_SIREN_64_64_3_L2_"))
    assert sorted(os.listdir(out)) == sorted(
        ["config.yaml", "images", "best_psnr_config.yaml", "best_ssim_config.yaml", "configs_and_results.txt",
         "results.json"] + ["hp_search_config_%d.yaml" % i for i in (1, 2, 3)])
    assert yaml.safe_load(open(os.path.join(out, "config.yaml"))) == BASE
    images = sorted(os.listdir(os.path.join(out, "images")))
    assert "train.png" in images and "train_kspace.png" in images and len(images) == 2 + 3 * MAX_EPOCH * 3
    for i in (1, 2, 3):
        for e in (1, 2):
            assert "config_%d_recon_kspace_%ddB.png" % (i, e) in images
            assert "config_%d_recon_kspace_%d_error.png" % (i, e) in images
            recon = [n for n in images if n.startswith("config_%d_recon_%d_" % (i, e)) and n.endswith("_ssim.png")]
            assert len(recon) == 1 and "_psnr_" in recon[0]
    for n in images:
        assert D.read_png_gray(os.path.join(out, "images", n)).shape == SHAPE[1:]
    rows = json.load(open(os.path.join(out, "results.json")))["results"]
    # the best epoch's picture carries the trial's best PSNR in its name
    for x in rows:
        e = x["best_psnr_ep"] + 1
        assert any(n.startswith("config_{}_recon_{}_{:.4g}_psnr_".format(x["index"], e, x["best_psnr"])) for n in images)
    # the same search without pictures and in one process: the same sampled configs, the same statistics
    r2 = _run_cli(args[:8] + ["--search-seed", 5])
    assert r2.returncode == 0, r2.stderr[-2000:]
    rows2 = json.load(open(os.path.join(json.loads(r2.stdout.strip().splitlines()[-1])["output_directory"],
                                        "results.json")))["results"]
    assert [{k: v for k, v in x.items() if k not in TIMING} for x in rows] == \
           [{k: v for k, v in x.items() if k not in TIMING} for x in rows2]
