#!/usr/bin/env python3
"""Wall clock of a hyperparameter search against the shell loop it replaces, on one MI355X -> profiles/hp_search.json.

Workload: 8 random-search trials on the headline shape (configs/config_siren_kspace.yaml: SIREN 5 x 256, batches of
25 000 rows) over a synthetic 15 x 640 x 368 k-space, 2 epochs with a validation after each; a second search space adds
``batch_size`` in {5 000, 10 000}.  Per workload:
  * python -m inr_mi355x.hp_search with --jobs 1, 2 and 4 (data cache on), and --jobs 1 with the cache off;
  * the baseline: the same 8 merged configs as 8 separate ``python -m inr_mi355x.train --val --synthetic ...`` commands
    of THIS tree, one after the other (what a user does without the search; that module's fit is the one the search
    calls, and the search left it as it was but for the inert ``model_seed=None``).
Worker scaling ("scaling" in the output): 8 trials end before every worker of --jobs 4 has left its first, slow fit, so
the same searches run again with 32 and 64 trials at --jobs 1, 2 and 4, without the baseline; the seconds per further
trial, (wall_64 - wall_32) / 32, are what a worker count costs once all workers are in their steady state.
Every child process runs under a timeout; the first one that fails ends the script (nothing else is started on the device).
    python tools/hp_search_bench.py [--out profiles/hp_search.json] [--trials 8] [--shape 15,640,368]
                                    [--part all|main|scaling] [--scaling-trials 32,64]
(--part main / scaling measures that part alone and keeps the other as the output file has it.)
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mri-implicit-neural-representations_amd")
sys.path.insert(0, PKG)

SPACES = {
    "batch_25000": {"lr": {"values": [1e-5, 1e-3], "type": "log"}, "encoder.scale": {"values": [2.0, 6.0], "type": "float"}},
    "batch_5000_10000": {"lr": {"values": [1e-5, 1e-3], "type": "log"},
                         "encoder.scale": {"values": [2.0, 6.0], "type": "float"},
                         "batch_size": {"values": [5000, 10000], "type": "item"}},
}
SEARCH_SEED = 0
MAX_EPOCH = 2


def run(cmd, timeout):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT]))
    t0 = time.time()
    r = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    wall = time.time() - t0
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit("{} ended with status {}: stopping here".format(" ".join(cmd[:4]), r.returncode))
    return wall, r.stdout


def search(base, extra, out_dir, timeout):
    """one search command -> its wall clock and what results.json says about every trial"""
    wall, stdout = run(base + ["--output_path", out_dir] + extra, timeout)
    line = json.loads(stdout.strip().splitlines()[-1])
    rows = json.load(open(os.path.join(line["output_directory"], "results.json")))["results"]
    return {"wall_seconds": wall, "ingests": line["ingests"],
            "setup_seconds": [r["setup_seconds"] for r in rows], "fit_seconds": [r["fit_seconds"] for r in rows],
            "steps": [r["steps"] for r in rows], "workers": [r["worker"] for r in rows],
            "best_psnr": [r["best_psnr"] for r in rows]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hp_search.json"))
    ap.add_argument("--trials", type=int, default=8)
    ap.add_argument("--shape", default="15,640,368")
    ap.add_argument("--timeout", type=float, default=600.0, help="seconds per child process")
    ap.add_argument("--part", choices=("all", "main", "scaling"), default="all")
    ap.add_argument("--scaling-trials", default="32,64", help="two trial counts of the worker-scaling searches")
    opts = ap.parse_args()
    from inr_mi355x import hp_search as HS
    from inr_mi355x.train import get_config, set_default_configs
    config_path = os.path.join(ROOT, "configs", "config_siren_kspace.yaml")
    config = set_default_configs(get_config(config_path))
    config.update(val_epoch=1, log_iter=100000)
    out = {}
    if opts.part != "all" and os.path.exists(opts.out):
        out = json.load(open(opts.out))
    out.update(shape=opts.shape, max_epoch=MAX_EPOCH, search_seed=SEARCH_SEED)
    few, many = (int(v) for v in opts.scaling_trials.split(","))
    with tempfile.TemporaryDirectory() as tmp:
        cfg_file = os.path.join(tmp, "config_siren_kspace.yaml")
        with open(cfg_file, "w") as f:
            yaml.safe_dump(config, f)
        if opts.part in ("all", "scaling"):
            out["scaling"] = {}
        for tag, space in SPACES.items() if opts.part in ("all", "scaling") else ():
            sc = out["scaling"][tag] = {"search_space": space, "trials": [few, many], "search": {}}
            for n in (few, many):
                hp_file = os.path.join(tmp, "%s_%d.yaml" % (tag, n))
                with open(hp_file, "w") as f:
                    yaml.safe_dump({"method": "random", "max_epoch": MAX_EPOCH, "num_search": n, "search_space": space}, f)
                base = [sys.executable, "-m", "inr_mi355x.hp_search", "--config", cfg_file, "--hp_config", hp_file,
                        "--synthetic", opts.shape, "--search-seed", str(SEARCH_SEED), "--trial-timeout", str(opts.timeout)]
                for jobs in (1, 2, 4):
                    name = "jobs%d_trials%d" % (jobs, n)
                    sc["search"][name] = search(base, ["--jobs", str(jobs)], os.path.join(tmp, "scaling", tag, name),
                                                opts.timeout)
                    print("scaling", tag, name, "%.2f s" % sc["search"][name]["wall_seconds"], flush=True)
            sc["seconds_per_further_trial"] = {
                "jobs%d" % j: (sc["search"]["jobs%d_trials%d" % (j, many)]["wall_seconds"]
                               - sc["search"]["jobs%d_trials%d" % (j, few)]["wall_seconds"]) / (many - few) for j in (1, 2, 4)}
        if opts.part in ("all", "main"):
            out.update(trials=opts.trials, workloads={})
        for tag, space in SPACES.items() if opts.part in ("all", "main") else ():
            hp = {"method": "random", "max_epoch": MAX_EPOCH, "num_search": opts.trials, "search_space": space}
            hp_file = os.path.join(tmp, tag + ".yaml")
            with open(hp_file, "w") as f:
                yaml.safe_dump(hp, f)
            w = out["workloads"][tag] = {"search_space": space, "search": {}}
            base = [sys.executable, "-m", "inr_mi355x.hp_search", "--config", cfg_file, "--hp_config", hp_file,
                    "--synthetic", opts.shape, "--search-seed", str(SEARCH_SEED), "--trial-timeout", str(opts.timeout)]
            for name, extra in (("jobs1", ["--jobs", "1"]), ("jobs1_cache_off", ["--jobs", "1", "--cache-bytes", "0"]),
                                ("jobs2", ["--jobs", "2"]), ("jobs4", ["--jobs", "4"])):
                w["search"][name] = search(base, extra, os.path.join(tmp, tag, name), opts.timeout)
                print(tag, name, "%.2f s" % w["search"][name]["wall_seconds"], flush=True)
            # the baseline: the same merged configs, one training command each
            hps = HS.expand_trials(hp, SEARCH_SEED)
            walls, fits, psnrs = [], [], []
            for i, merged in enumerate(HS.merged_configs(config, hps)):
                one = os.path.join(tmp, "%s_trial_%d.yaml" % (tag, i + 1))
                with open(one, "w") as f:
                    yaml.safe_dump(HS.trial_config(merged, MAX_EPOCH), f)
                wall, stdout = run([sys.executable, "-m", "inr_mi355x.train", "--config", one, "--val", "--synthetic",
                                    opts.shape, "--output_path", os.path.join(tmp, tag, "loop_%d" % (i + 1))], opts.timeout)
                res = json.loads(stdout.strip().splitlines()[-1])
                walls.append(wall)
                fits.append(res["seconds"])
                psnrs.append(res["best_psnr"])
            w["train_cli_loop"] = {"wall_seconds": sum(walls), "per_command_seconds": walls, "fit_seconds": fits,
                                   "best_psnr": psnrs}
            print(tag, "train_cli_loop", "%.2f s" % sum(walls), flush=True)
    os.makedirs(os.path.dirname(opts.out), exist_ok=True)
    with open(opts.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({t: dict({k: round(v["wall_seconds"], 2) for k, v in w["search"].items()},
                              train_cli_loop=round(w["train_cli_loop"]["wall_seconds"], 2))
                      for t, w in out.get("workloads", {}).items()}))
    print(json.dumps({t: {k: round(v, 4) for k, v in sc["seconds_per_further_trial"].items()}
                      for t, sc in out.get("scaling", {}).items()}))


if __name__ == "__main__":
    main()
