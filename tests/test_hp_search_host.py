"""Host logic of the hyperparameter search (inr_mi355x/hp_search.py) on the CPU: search-space expansion against what the
reference's own find_best_config.py produced (tests/golden/hp_search.json, written by tools/make_golden.py), the
running config of update_model_config, the choice and the files of the best configs, the refusals, the data cache and the
worker processes' failure rule.  Trials are stubs (``run_trial=`` in process, a small script speaking the line protocol
as a worker): no library, no GPU."""
import contextlib
import copy
import io
import json
import os
import sys
import textwrap

import pytest
import torch
import yaml

from conftest import GOLDEN, PKG, ROOT

from inr_mi355x import hp_search as HS

GOLD = json.load(open(os.path.join(GOLDEN, "hp_search.json")))
BASE = GOLD["base_config"]


def quiet(fn, *a, **k):
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        res = fn(*a, **k)
    return res, out.getvalue()


def same_bits(a, b) -> bool:
    """equal, with floats compared by their bits and ints not passing for floats"""
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same_bits(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    if isinstance(a, float) or isinstance(b, float):
        return type(a) is type(b) and a.hex() == b.hex()
    return type(a) is type(b) and a == b


# ---- search spaces against the reference's -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", GOLD["random"], ids=lambda c: "seed%d" % c["seed"])
def test_random_sampling_reproduces_the_reference(case):
    hp = {"method": "random", "max_epoch": 2, "num_search": case["num_search"],
          "search_space": copy.deepcopy(case["search_space"])}
    configs, printed = quiet(HS.expand_trials, hp, case["seed"])
    assert same_bits(configs, case["configs"]), (configs, case["configs"])
    assert same_bits(HS.merged_configs(BASE, configs), case["merged"])
    assert hp["search_space"] == case["search_space"]  # the caller's dict is left alone
    for key, spec in case["search_space"].items():
        if spec["type"] not in HS.ALLOWED_RANDOM_SEARCH_PARAMS:
            assert all(key not in c for c in configs)
            assert printed.count("'{}' is not a valid random sampling mode. Ignoring hyper-param '{}'".format(
                spec["type"], key)) == case["num_search"]
        elif spec["type"] == "log" and min(spec["values"][0], spec["values"][-1]) <= 0:
            assert all(key not in c for c in configs)
            assert printed.count("Invalid value encountered for logarithmic sampling of '{}'. Ignoring this hyper "
                                 "param.".format(key)) == case["num_search"]
        else:
            assert all(key in c for c in configs)


def test_fixture_holds_the_invalid_cases():
    types = [(s["type"], s["values"]) for c in GOLD["random"] for s in c["search_space"].values()]
    assert any(t not in HS.ALLOWED_RANDOM_SEARCH_PARAMS for t, _ in types)
    assert any(t == "log" and v[0] <= 0 for t, v in types)


def test_search_seed_none_seeds_nothing():
    import random
    hp = {"method": "random", "max_epoch": 1, "num_search": 2, "search_space": GOLD["random"][3]["search_space"]}
    random.seed(GOLD["random"][3]["seed"])
    first, _ = quiet(HS.expand_trials, hp, None)
    second, _ = quiet(HS.expand_trials, hp, None)  # goes on in the ambient stream: the fixture's third and fourth draws
    assert same_bits(first, GOLD["random"][3]["configs"][:2]) and same_bits(second, GOLD["random"][3]["configs"][2:4])


@pytest.mark.parametrize("case", GOLD["grid"], ids=["2x2", "2x3x1"])
def test_grid_order_equals_the_reference(case):
    hp = {"method": "grid", "max_epoch": 2, "search_space": copy.deepcopy(case["search_space"])}
    configs = HS.expand_trials(hp)
    assert same_bits(configs, case["configs"])
    assert same_bits(HS.merged_configs(BASE, configs), case["merged"])


def test_update_model_config_nested_cumulative_and_copied():
    base = copy.deepcopy(BASE)
    hps = [{"lr": 0.5, "net.network_width": 128}, {"encoder.scale": 9}, {"lr": 0.25}]
    merged = HS.merged_configs(base, hps)
    assert base == BASE  # the caller's config is not the running dict
    assert [m["lr"] for m in merged] == [0.5, 0.5, 0.25]  # a key skipped in trial i keeps trial i-1's value
    assert [m["net"]["network_width"] for m in merged] == [128, 128, 128]
    assert [m["encoder"]["scale"] for m in merged] == [BASE["encoder"]["scale"], 9, 9]
    assert [m["config_index"] for m in merged] == [1, 2, 3]
    assert len({id(m) for m in merged}) == 3 and len({id(m["net"]) for m in merged}) == 3
    merged[0]["net"]["network_width"] = -1
    assert merged[1]["net"]["network_width"] == 128
    # one dot, two levels: the in-place function of the reference
    d = {"a": {"b": 1}, "c": 2}
    assert HS.update_model_config(d, {"a.b": 5, "c": 6, "e": 7}) is d and d == {"a": {"b": 5}, "c": 6, "e": 7}
    t = HS.trial_config(merged[1], 7)
    assert t["max_epoch"] == 7 and merged[1]["max_epoch"] == BASE["max_epoch"] and t["net"] is not merged[1]["net"]


# ---- best configs and files, with stub statistics ----------------------------------------------------------------------
def stub_source(calls):
    def source(cfg):
        calls.append(cfg.get("normalization"))
        return torch.zeros(100, 2), torch.zeros(100, 3), (1, 10, 10)
    return source


def grid_hp(**space):
    return {"method": "grid", "max_epoch": 2,
            "search_space": {k: {"values": v, "type": "item"} for k, v in space.items()}}


def stats(psnr, ssim, ep=1):
    return {"best_psnr": psnr, "best_psnr_ep": ep, "best_ssim": ssim, "best_ssim_ep": ep}


def test_best_files_hold_the_winners_not_the_last_trial(tmp_path):
    table = {1e-4: stats(20.0, 0.5), 2e-4: stats(31.0, 0.6), 3e-4: stats(31.0, 0.9), 4e-4: {"error": "refused"},
             5e-4: stats(25.0, 0.9)}
    seen = []

    def run_trial(cfg, max_epoch, data):
        seen.append((cfg["config_index"], max_epoch, data[2]))
        return table[cfg["lr"]]

    calls = []
    res, printed = quiet(HS.run_search, BASE, grid_hp(lr=list(table)), str(tmp_path), source=stub_source(calls),
                         run_trial=run_trial)
    assert seen == [(i + 1, 2, (1, 10, 10)) for i in range(5)]
    # strict '>': the tie at 31.0 keeps trial 2, the tie at 0.9 keeps trial 3; the last trial wins nothing
    assert res["best_psnr"]["index"] == 2 and res["best_psnr"]["value"] == 31.0
    assert res["best_ssim"]["index"] == 3 and res["best_ssim"]["value"] == 0.9
    bp = yaml.safe_load(open(tmp_path / "best_psnr_config.yaml"))
    bs = yaml.safe_load(open(tmp_path / "best_ssim_config.yaml"))
    assert bp["lr"] == 2e-4 and bp["config_index"] == 2 and bs["lr"] == 3e-4 and bs["config_index"] == 3
    assert bp["net"] == BASE["net"] and bp["max_epoch"] == BASE["max_epoch"]
    assert not res["aborted"] and res["ingests"] == 1 and calls == ["coil"]
    # the reference's file names, one line per trial, machine-readable records in trial order
    names = sorted(os.listdir(tmp_path))
    assert names == sorted(["best_psnr_config.yaml", "best_ssim_config.yaml", "configs_and_results.txt", "results.json"]
                           + ["hp_search_config_%d.yaml" % i for i in range(1, 6)])
    assert yaml.safe_load(open(tmp_path / "hp_search_config_4.yaml")) == {"lr": 4e-4}
    lines = open(tmp_path / "configs_and_results.txt").read().splitlines()
    assert len(lines) == 5 and lines[0] == "{} -> {}".format({"lr": 1e-4}, stats(20.0, 0.5))
    assert lines[3] == "{} -> {}".format({"lr": 4e-4}, {"error": "refused"})
    js = json.load(open(tmp_path / "results.json"))
    assert js["aborted"] is False and [r["index"] for r in js["results"]] == [1, 2, 3, 4, 5]
    assert js["results"][3]["error"] == "refused" and js["results"][1]["best_psnr"] == 31.0
    assert js["results"][1]["hp"] == {"lr": 2e-4} and js["results"][1]["worker"] == 0
    assert "** Running Grid Search **" in printed and "Evaluating Config #5 [of 5]" in printed


def test_error_trials_never_win(tmp_path):
    res, _ = quiet(HS.run_search, BASE, grid_hp(lr=[1e-4, 2e-4]), str(tmp_path), source=stub_source([]),
                   run_trial=lambda cfg, e, d: {"error": "no kernel"})
    assert res["best_psnr"] is None and res["best_ssim"] is None and not res["aborted"]
    assert yaml.safe_load(open(tmp_path / "best_psnr_config.yaml")) is None
    # a trial without a validation epoch keeps the reference's initial values: it cannot win either ('>' is strict)
    res, _ = quiet(HS.run_search, BASE, grid_hp(lr=[1e-4]), str(tmp_path), source=stub_source([]),
                   run_trial=lambda cfg, e, d: dict(HS.INITIAL_STATS))
    assert res["best_psnr"] is None and res["results"][0]["best_psnr"] == -999999 and res["results"][0]["best_ssim"] == -1


def test_other_failures_end_the_search_at_once(tmp_path):
    seen = []

    def run_trial(cfg, max_epoch, data):
        seen.append(cfg["config_index"])
        if cfg["config_index"] == 2:
            raise RuntimeError("libinr_mi355x: error -3: launch failed")
        return stats(20.0, 0.5)

    with pytest.raises(RuntimeError, match="launch failed"):
        quiet(HS.run_search, BASE, grid_hp(lr=[1e-4, 2e-4, 3e-4]), str(tmp_path), source=stub_source([]),
              run_trial=run_trial)
    assert seen == [1, 2]
    js = json.load(open(tmp_path / "results.json"))
    assert js["aborted"] is True and [r["index"] for r in js["results"]] == [1]
    with pytest.raises(RuntimeError, match="returned"):  # neither a result nor a recorded refusal
        quiet(HS.run_search, BASE, grid_hp(lr=[1e-4]), str(tmp_path), source=stub_source([]),
              run_trial=lambda cfg, e, d: {"best_psnr": 1.0})


@pytest.mark.parametrize("name", ["MultiscaleKFourier", "MultiscaleBoundedFourier", "BoundedFourier"])
def test_multiscale_models_are_refused_before_any_trial(tmp_path, name):
    ran = []
    with pytest.raises(NotImplementedError, match="single-scale"):
        quiet(HS.run_search, dict(BASE, model=name), grid_hp(lr=[1e-4]), str(tmp_path), source=stub_source(ran),
              run_trial=lambda *a: ran.append(1))
    with pytest.raises(NotImplementedError, match="single-scale"):
        quiet(HS.run_search, BASE, grid_hp(model=["SIREN", name]), str(tmp_path), source=stub_source(ran),
              run_trial=lambda *a: ran.append(1))
    assert not ran and not os.listdir(tmp_path)


def test_lsl_is_refused_before_any_trial(tmp_path):
    ran = []
    with pytest.raises(NotImplementedError, match="LSL"):
        quiet(HS.run_search, dict(BASE, loss="LSL"), grid_hp(lr=[1e-4]), str(tmp_path), source=stub_source(ran),
              run_trial=lambda *a: ran.append(1))
    with pytest.raises(NotImplementedError, match="LSL"):
        quiet(HS.run_search, BASE, grid_hp(loss=["L2", "LSL"]), str(tmp_path), source=stub_source(ran),
              run_trial=lambda *a: ran.append(1))
    assert not ran and not os.listdir(tmp_path)


# ---- data cache ---------------------------------------------------------------------------------------------------------
def test_cache_one_ingest_per_distinct_key_and_again_after_eviction(tmp_path):
    calls = []
    cache = HS.DataCache(stub_source(calls))
    a = cache.get(dict(BASE, normalization="coil", lr=1.0))
    assert cache.get(dict(BASE, normalization="coil", lr=2.0, batch_size=7))[0] is a[0]  # not data keys
    b = cache.get(dict(BASE, normalization="max"))
    assert b[0] is not a[0] and cache.get(dict(BASE, normalization="coil"))[0] is a[0]
    assert cache.ingests == 2 and calls == ["coil", "max"]
    for k in HS.DATA_KEYS:  # every data key makes a new entry
        n = cache.ingests
        cache.get(dict(BASE, **{k: "other"}))
        assert cache.ingests == n + 1, k
    assert HS.DataCache(stub_source([]), extra_key=(4, 64, 48)).get(BASE)[2] == (1, 10, 10)
    # one entry is 100 * (2 + 3) * 4 = 2000 bytes: a budget of 3000 holds one, so coil is ingested again after max
    calls = []
    small = HS.DataCache(stub_source(calls), budget=3000)
    for n in ("coil", "coil", "max", "coil", "max"):
        small.get(dict(BASE, normalization=n))
    assert calls == ["coil", "max", "coil", "max"] and small.ingests == 4 and len(small.entries) == 1
    # least recently used goes first
    calls = []
    lru = HS.DataCache(stub_source(calls), budget=4000)
    for n in ("coil", "max", "coil", "none", "coil", "max"):
        lru.get(dict(BASE, normalization=n))
    assert calls == ["coil", "max", "none", "max"]
    assert HS.CACHE_BUDGET_BYTES == 8 << 30
    # through the search: the interleaved grid still ingests each normalisation once, and `ingests` reports it
    calls = []
    res, _ = quiet(HS.run_search, BASE, grid_hp(lr=[1e-4, 2e-4], normalization=["coil", "max"]), str(tmp_path),
                   source=stub_source(calls), run_trial=lambda cfg, e, d: stats(1.0, 0.1))
    assert res["ingests"] == 2 and calls == ["coil", "max"]
    calls = []
    res, _ = quiet(HS.run_search, BASE, grid_hp(lr=[1e-4, 2e-4], normalization=["coil", "max"]), str(tmp_path),
                   source=stub_source(calls), run_trial=lambda cfg, e, d: stats(1.0, 0.1), cache_bytes=0)
    assert res["ingests"] == 4 and calls == ["coil", "max", "coil", "max"]


# ---- worker processes, with a CPU stub worker ------------------------------------------------------------------------
STUB = textwrap.dedent('''
    import json, sys, time
    mode, at = sys.argv[1], int(sys.argv[2])
    setup = json.loads(sys.stdin.readline())["setup"]
    assert setup["max_epoch"] == 2
    for line in sys.stdin:
        msg = json.loads(line)
        i, cfg = msg["trial"], msg["config"]
        if i == at and mode == "exit3":
            sys.exit(3)
        if i == at and mode == "garbage":
            print("not a protocol line", flush=True)
            continue
        if i == at and mode == "hang":
            time.sleep(60)
        if mode != "ok":
            time.sleep(0.5)
        res = {"best_psnr": 20.0 + 1e4 * cfg["lr"], "best_psnr_ep": 1, "best_ssim": 1.0 - 1e3 * cfg["lr"],
               "best_ssim_ep": 0, "steps": 4, "fit_seconds": 0.01, "setup_seconds": 0.02, "ingests": 1}
        if cfg["lr"] == 3e-4:
            res = {"error": "refused", "ingests": 1}
        print(json.dumps({"trial": i, "result": res}), flush=True)
''')


def stub_trial(cfg, max_epoch, data):
    if cfg["lr"] == 3e-4:
        return {"error": "refused"}
    return {"best_psnr": 20.0 + 1e4 * cfg["lr"], "best_psnr_ep": 1, "best_ssim": 1.0 - 1e3 * cfg["lr"],
            "best_ssim_ep": 0, "steps": 4}


def worker_cmd(tmp_path, mode="ok", at=-1):
    p = tmp_path / "stub_worker.py"
    p.write_text(STUB)
    return [sys.executable, str(p), mode, str(at)]


LRS = [1e-4, 2e-4, 3e-4, 4e-4, 5e-4, 6e-4]
UNTIMED = ("index", "hp", "error") + HS.STAT_KEYS + ("steps",)


def untimed(rows):
    return [{k: r[k] for k in UNTIMED if k in r} for r in rows]


@pytest.mark.parametrize("jobs", [2, 3])
def test_results_do_not_depend_on_jobs(tmp_path, jobs):
    one, _ = quiet(HS.run_search, BASE, grid_hp(lr=LRS), str(tmp_path), source=stub_source([]), run_trial=stub_trial)
    d = tmp_path / "par"
    d.mkdir()
    par, _ = quiet(HS.run_search, BASE, grid_hp(lr=LRS), str(d), jobs=jobs, worker_cmd=worker_cmd(tmp_path),
                   trial_timeout=60)
    assert not par["aborted"] and [r["index"] for r in par["results"]] == [1, 2, 3, 4, 5, 6]
    assert untimed(par["results"]) == untimed(one["results"])
    assert {r["worker"] for r in par["results"]} <= set(range(jobs))
    assert par["best_psnr"]["index"] == one["best_psnr"]["index"] == 6
    assert par["best_ssim"]["index"] == one["best_ssim"]["index"] == 1
    assert par["ingests"] == len({r["worker"] for r in par["results"]})
    for name in ("best_psnr_config.yaml", "best_ssim_config.yaml", "configs_and_results.txt"):
        assert open(d / name).read() == open(tmp_path / name).read()
    assert untimed(json.load(open(d / "results.json"))["results"]) == untimed(one["results"])


@pytest.mark.parametrize("mode", ["exit3", "garbage", "hang"])
def test_a_failing_child_stops_the_dispatch(tmp_path, mode):
    """Trial 2 (0-based 1) goes to the second worker at once and fails there; the first worker's running trial finishes;
    whatever it was handed before the failure was seen (trial 3 at most) finishes too; nothing else is started and
    nothing is retried."""
    res, _ = quiet(HS.run_search, BASE, grid_hp(lr=LRS), str(tmp_path), jobs=2, worker_cmd=worker_cmd(tmp_path, mode, 1),
                   trial_timeout=3.0 if mode == "hang" else 60)
    got = [r["index"] for r in res["results"]]
    assert res["aborted"] and 1 in got and 2 not in got, (got, res["reason"])
    if mode != "hang":  # (a hung child is only known to have failed once its time is up: the other worker goes on till then)
        assert set(got) <= {1, 3}, got
    js = json.load(open(tmp_path / "results.json"))
    assert js["aborted"] is True and [r["index"] for r in js["results"]] == got and js["trials"] == 6
    assert {"exit3": "status 3", "garbage": "answered trial 2", "hang": "past 3 s"}[mode] in js["reason"]


def test_cli_exits_non_zero_after_a_failed_child(tmp_path, monkeypatch):
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(yaml.safe_dump(BASE))
    hp = tmp_path / "hp.json"
    hp.write_text(json.dumps(grid_hp(lr=LRS)))  # the reference's hp files are JSON: YAML reads them
    args = ["--config", str(cfg), "--hp_config", str(hp), "--output_path", str(tmp_path / "out"), "--jobs", "2"]
    monkeypatch.setattr(HS, "WORKER_CMD", tuple(worker_cmd(tmp_path, "exit3", 1)))  # the command main() starts workers with
    rc, _ = quiet(HS.main, args)
    assert rc == 1
    monkeypatch.setattr(HS, "WORKER_CMD", tuple(worker_cmd(tmp_path)))
    rc, printed = quiet(HS.main, args)
    assert rc == 0
    line = json.loads(printed.strip().splitlines()[-1])
    assert line["trials"] == 6 and not line["aborted"] and line["best_psnr"]["index"] == 6
    out = line["output_directory"]
    assert os.path.relpath(out, tmp_path).startswith(os.path.join("out", "outputs", "cfg", "synthetic", "img_SIREN_64_64_3_L2_"))
    assert "_hp_grid_search__scale2_size32" in out
    assert yaml.safe_load(open(os.path.join(out, "config.yaml"))) == BASE


def test_jobs_cap(tmp_path):
    assert HS.MAX_JOBS == 8
    for jobs in (0, 9, 16):
        with pytest.raises(ValueError, match="jobs"):
            HS.run_search(BASE, grid_hp(lr=LRS), str(tmp_path), jobs=jobs, worker_cmd=worker_cmd(tmp_path))
    with pytest.raises(ValueError, match="fresh processes"):
        HS.run_search(BASE, grid_hp(lr=LRS), str(tmp_path), jobs=2, run_trial=stub_trial)
    with pytest.raises(SystemExit):
        with contextlib.redirect_stderr(io.StringIO()):
            HS.main(["--config", "x", "--hp_config", "y", "--jobs", "9"])


def test_model_seed_none_changes_nothing_and_42_reseeds():
    """INRTrainer(model_seed=...) on the constructors alone (the trainer itself needs the library): the RNG order it
    follows -- encoder from `seed`, torch.manual_seed(model_seed), model -- gives the fixture's hashes."""
    import hashlib
    import inspect
    import inr_mi355x as M
    from inr_mi355x.train import INRTrainer
    sig = inspect.signature(INRTrainer.__init__)
    assert sig.parameters["model_seed"].default is None
    torch.manual_seed(0)
    M.Positional_Encoder(BASE["encoder"], device="cpu")
    torch.manual_seed(GOLD["init_seed"])
    sd = M.SIREN(GOLD["init"]["SIREN"]["net"]).state_dict()
    for k, v in sd.items():
        assert hashlib.sha256(v.detach().numpy().tobytes()).hexdigest() == GOLD["init"]["SIREN"]["sha256"][k], k


# ---- what ships with the repository -------------------------------------------------------------------------------------
def shipped_pairs():
    """(config, hp file) pairs the documents put on one command line: README.md and the header of every configs/hp_*.yaml"""
    import glob
    import re
    texts = [open(os.path.join(ROOT, "README.md")).read()]
    texts += [open(p).read() for p in sorted(glob.glob(os.path.join(ROOT, "configs", "hp_*.yaml")))]
    pairs = set()
    for text in texts:
        for m in re.finditer(r"--config\s+(\S+)\s+--hp_config\s+(\S+)", text):
            pairs.add((m.group(1), m.group(2)))
    return sorted(pairs)


def test_shipped_example_scores_its_trials():
    """The documented command must score trials: at least one validation epoch ((epoch + 1) % val_epoch == 0, the rule of
    INRTrainer.fit) inside the hp file's max_epoch, for every value of val_epoch the search can set."""
    from inr_mi355x.train import get_config, set_default_configs
    pairs = shipped_pairs()
    assert ("configs/config_siren_kspace.yaml", "configs/hp_siren_random.yaml") in pairs
    for cfg_path, hp_path in pairs:
        config = set_default_configs(get_config(os.path.join(ROOT, cfg_path)))
        hp = get_config(os.path.join(ROOT, hp_path))
        HS.check_search(config, hp)
        searched = (hp["search_space"].get("val_epoch") or {}).get("values")
        for val_epoch in searched or [config["val_epoch"]]:
            scored = [e for e in range(int(hp["max_epoch"])) if (e + 1) % int(val_epoch) == 0]
            assert scored, "{} with {}: no validation epoch within max_epoch={} (val_epoch={})".format(
                hp_path, cfg_path, hp["max_epoch"], val_epoch)
        trials, _ = quiet(HS.expand_trials, hp, 0)
        assert len(trials) == (hp["num_search"] if hp["method"] == "random" else len(trials)) > 0
        assert len(HS.merged_configs(config, trials)) == len(trials)


def test_unsupported_is_returned_before_any_launch():
    """_lib.check() raises INR_ERR_UNSUPPORTED as NotImplementedError and the search records that as a refusal: the
    library must return that code from plan creation alone, before anything runs on the device."""
    import glob
    import re
    hits = 0
    for path in sorted(glob.glob(os.path.join(PKG, "csrc", "*"))):
        if not os.path.isfile(path) or not path.endswith((".hip", ".h", ".hpp", ".cpp")):
            continue
        text = open(path, errors="replace").read()
        for m in re.finditer(r"fail\(\s*INR_ERR_UNSUPPORTED\s*,\s*\"([^\"]*)", text):
            hits += 1
            assert m.group(1).startswith("inr_plan_create:"), (os.path.basename(path), m.group(1))
        assert len(re.findall(r"INR_ERR_UNSUPPORTED", text)) == len(re.findall(r"fail\(\s*INR_ERR_UNSUPPORTED", text)), path
    assert hits > 0
