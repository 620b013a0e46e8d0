"""Hyperparameter search driver: the reference's hp_search_script.py:12-83, parameter_search/find_best_config.py and
parameter_search/hp_model_training.py:13-228 over the fused MI355X engine.  A grid or random search over config keys
('lr', 'net.*', 'encoder.*', 'batch_size', 'normalization', ...) trains every candidate for the hp file's ``max_epoch``
epochs, validates every config['val_epoch'] epochs and writes best_psnr_config.yaml / best_ssim_config.yaml.

Kept from the reference: the search-space file format ({method, max_epoch, num_search, search_space: {key: {values,
type}}}), grid order (itertools.product in key order), the random sampler (one draw per key, in key order, from Python's
``random``), update_model_config's one-dot split and its running dict (a key skipped in trial i keeps trial i-1's
value), torch.manual_seed(42) between the encoder's and the model's construction, the output tree and file names.
Changed, on purpose: the best files hold a copy of the config that won (the reference writes the dict it
keeps mutating: the LAST trial's), configs_and_results.txt has one line per trial (the reference's list is never
appended to), results.json, loss 'LSL' is refused up front, a trial the engine has no kernel for is recorded as
{"error": ...} and the search goes on, any other failure ends it.

What this driver adds over a shell loop of ``python -m inr_mi355x.train --val``: one process, so one library load; one
ingest per distinct dataset (DataCache: the device tensors stay in HBM between trials); ``--jobs N`` fresh worker
processes that run trials side by side.  A trial's hot path is the existing fused step, validation
sweep and metric / display kernels.

CLI:
    python -m inr_mi355x.hp_search --config cfg.yaml --hp_config hp.yaml [--output_path out] [--synthetic C,H,W]
                                   [--seed S] [--search-seed N] [--jobs N] [--save-images] [--trial-timeout SECONDS]
                                   [--band-report [N]]
(--trial-timeout limits a worker process's trial, so it needs --jobs > 1: with --jobs 1 the trials run in the command's
own process and are not limited.)
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import random
import select
import subprocess
import sys
import time
from collections import OrderedDict
from datetime import datetime
from itertools import product
from math import log10
from typing import Callable, Optional

import yaml

# find_best_config.py:11
ALLOWED_RANDOM_SEARCH_PARAMS = ["log", "int", "float", "item"]
# hp_model_training.py:51-66: the single-scale models; anything else is `raise NotImplementedError` there
SEARCH_MODELS = ("SIREN", "WIRE", "WIRE2D", "FFN", "Fourier", "Gabor", "KGabor")
MODEL_SEED = 42  # hp_model_training.py:49
# hp_model_training.py:112-115
INITIAL_STATS = {"best_psnr": -999999, "best_psnr_ep": 0, "best_ssim": -1, "best_ssim_ep": 0}
STAT_KEYS = tuple(INITIAL_STATS)
# The config keys that decide what the source returns (find_best_config.py:57-72 hands these to get_data_loader;
# batch_size only shapes the loader there, and the trainers apply 'undersampling' / 'per_coil' to the resident tensors
# themselves -- they stay in the key so that a source which does look at them is never served a stale entry).
DATA_KEYS = ("data", "data_root", "set", "sample", "slice", "custom_file_or_path", "transform", "normalization",
             "full_norm", "undersampling", "per_coil", "virtual_coils")
CACHE_BUDGET_BYTES = 8 << 30  # resident datasets kept between trials; least recently used ones go first above it
# Worker processes per search.  The GPU boxes are shared and allow 16 processes with the device open in total: a search
# takes at most half of them, and at 25 000-row batches 196 of 256 CUs are busy already (README, Switches).
MAX_JOBS = 8
# Seconds a WORKER may spend on one trial (--jobs > 1) before the parent kills it.  With --jobs 1 the trials run in the
# calling process, which nothing watches: no limit applies there.
TRIAL_TIMEOUT = 3600.0
WORKER_CMD = (sys.executable, "-m", "inr_mi355x.hp_search", "--worker")


# ---- search spaces (find_best_config.py) ------------------------------------------------------------------------------
def update_model_config(model_configs: dict, hp_configs: dict) -> dict:
    """find_best_config.py:14-25: in place; 'a.b' sets model_configs['a']['b'] (one dot, two levels)."""
    for k in hp_configs:
        k_split = k.split(".")
        if "." in k:
            model_configs[k_split[0]][k_split[1]] = hp_configs[k]
        else:
            model_configs[k] = hp_configs[k]
    return model_configs


def grid_search_configs(search_space: dict) -> list:
    """find_best_config.py:136-148: every combination of the 'values' lists, in key order."""
    values = {k: v.get("values") for k, v in search_space.items()}
    return [dict(zip(values.keys(), instance)) for instance in product(*values.values())]


def random_search_spaces_to_config(random_search_spaces: dict) -> dict:
    """find_best_config.py:187-214: one draw per key, in key order, from Python's ``random``; the reference's two
    messages for an unknown mode and for a non-positive 'log' bound, whose keys are left out."""
    config = {}
    for key, (rng, mode) in random_search_spaces.items():
        if mode not in ALLOWED_RANDOM_SEARCH_PARAMS:
            print("'{}' is not a valid random sampling mode. "
                  "Ignoring hyper-param '{}'".format(mode, key))
        elif mode == "log":
            if rng[0] <= 0 or rng[-1] <= 0:
                print("Invalid value encountered for logarithmic sampling "
                      "of '{}'. Ignoring this hyper param.".format(key))
                continue
            sample = random.uniform(log10(rng[0]), log10(rng[-1]))
            config[key] = 10 ** (sample)
        elif mode == "int":
            config[key] = random.randint(rng[0], rng[-1])
        elif mode == "float":
            config[key] = random.uniform(rng[0], rng[-1])
        elif mode == "item":
            config[key] = random.choice(rng)
    return config


def random_search_configs(search_space: dict, num_search: int) -> list:
    """find_best_config.py:178-182."""
    spaces = {k: (v.get("values"), v.get("type")) for k, v in search_space.items()}
    return [random_search_spaces_to_config(spaces) for _ in range(num_search)]


def expand_trials(hp_config: dict, search_seed: Optional[int] = None) -> list:
    """The hp dict of every trial (hp_search_script.py:44-57).  ``search_seed``: random.seed() before sampling (the
    reference is unseeded; None seeds nothing)."""
    if hp_config["method"] == "grid":
        return grid_search_configs(hp_config["search_space"])
    if search_seed is not None:
        random.seed(search_seed)
    return random_search_configs(hp_config["search_space"], hp_config["num_search"])


def merged_configs(config: dict, hp_configs: list) -> list:
    """The model config of every trial: update_model_config applied to ONE running dict in trial order, as
    find_best_config.py:49-50 does (with its 1-based 'config_index'), each record a deep copy of its own."""
    running = copy.deepcopy(config)
    out = []
    for i, hp in enumerate(hp_configs):
        running = update_model_config(running, hp)
        running["config_index"] = i + 1
        out.append(copy.deepcopy(running))
    return out


def trial_config(merged: dict, max_epoch: int) -> dict:
    """What a trial's trainer is built from: the merged config with max_epoch replaced by the hp file's (the
    reference's LambdaLR and epoch loop take that value, hp_model_training.py:119-121)."""
    return dict(copy.deepcopy(merged), max_epoch=int(max_epoch))


def check_search(config: dict, hp_config: dict) -> None:
    """Refusals before the first trial: models outside hp_model_training.py:51-66, loss 'LSL' (validate() refuses it),
    an unknown method."""
    space = hp_config.get("search_space") or {}
    if hp_config.get("method") not in ("grid", "random"):
        raise ValueError(f"hp config: method {hp_config.get('method')!r} (grid | random)")
    for name in [config.get("model")] + list((space.get("model") or {}).get("values") or []):
        if name not in SEARCH_MODELS:
            raise NotImplementedError(f"hp search: model {name!r} (the search trains single-scale models only: "
                                      f"{', '.join(SEARCH_MODELS)}; hp_model_training.py:51-66)")
    for name in [config.get("loss")] + list((space.get("loss") or {}).get("values") or []):
        if name == "LSL":
            raise NotImplementedError("hp search: loss 'LSL' (CenterLoss): every trial is scored by validation epochs, "
                                      "which refuse it")


# ---- one ingest per distinct dataset ----------------------------------------------------------------------------------
def data_key(config: dict) -> tuple:
    return tuple(repr(config.get(k)) for k in DATA_KEYS)


class DataCache:
    """Keeps what ``source(cfg)`` returned -- (image, coords, shape) -- per data_key(cfg), on ``device`` when one is
    given.  Least-recently-used entries are dropped while the tensors held exceed ``budget`` bytes (an entry larger than
    the budget is handed out and not kept).  ``ingests`` counts the source calls."""

    def __init__(self, source: Callable, budget: int = CACHE_BUDGET_BYTES, device=None, extra_key: tuple = ()):
        self.source, self.budget, self.device, self.extra_key = source, int(budget), device, tuple(extra_key)
        self.entries = OrderedDict()
        self.ingests = 0

    @staticmethod
    def _bytes(entry) -> int:
        return sum(t.numel() * t.element_size() for t in entry[:2])

    def get(self, config: dict):
        key = self.extra_key + data_key(config)
        if key in self.entries:
            self.entries.move_to_end(key)
            return self.entries[key]
        got = self.source(config)
        image, coords, shape = got[:3]
        self.ingests += 1
        if self.device is not None:
            image, coords = image.to(self.device).contiguous(), coords.to(self.device).contiguous()
        entry = (image, coords, tuple(int(v) for v in shape[:3]))
        if len(got) > 3 and got[3] is not None:  # config['virtual_coils']: the compression the data came through
            entry = entry + (got[3],)
        self.entries[key] = entry
        while self.entries and sum(self._bytes(e) for e in self.entries.values()) > self.budget:
            self.entries.popitem(last=False)
        return entry


def synthetic_source(C: int, H: int, W: int) -> Callable:
    """--synthetic C,H,W: make_kspace with the trial's 'normalization' and 'transform', as inr_mi355x.train does."""
    def source(cfg):
        if cfg.get("virtual_coils"):
            import argparse
            from .cli import cli_fit_data
            return cli_fit_data(argparse.Namespace(synthetic=f"{C},{H},{W}"), cfg, "coil",
                                image_space=bool(cfg.get("transform", False)))
        from .synthetic import make_kspace
        return make_kspace(C, H, W, normalization=cfg.get("normalization", "coil"),
                           image_space=bool(cfg.get("transform", False)))
    return source


def dataset_source(cfg):
    """find_best_config.py:56-72: the scan the config names."""
    from .datasets import from_config, trainer_inputs
    ds = from_config(cfg, "cuda")
    return (*trainer_inputs(ds), ds.coil_compression)


# ---- one trial (hp_model_training.py:13-228) --------------------------------------------------------------------------
def build_trial_trainer(cfg: dict, data, seed: int = 0, device="cuda"):
    """The trainer of a trial: encoder from ``seed``, model from torch.manual_seed(42) (hp_model_training.py:46-49)."""
    from .train import INRTrainer
    image, coords, shape = data[:3]
    return INRTrainer(cfg, image, coords, shape, device, seed=seed, model_seed=MODEL_SEED,
                      coil_compression=data[3] if len(data) > 3 else None)


def hp_training_function(config: dict, max_epoch: int, data, *, seed: int = 0, image_directory: Optional[str] = None,
                         device="cuda", band_report=None) -> dict:
    """Fits ``config`` (a merged config; its 'config_index' names the pictures) for ``max_epoch`` epochs with a
    validation every config['val_epoch'] epochs and returns {best_psnr, best_psnr_ep, best_ssim, best_ssim_ep} (initial
    values and strict '>' of hp_model_training.py:112-115,202-207) plus 'steps', 'fit_seconds' and 'build_seconds'.  A trainer
    construction that raises NotImplementedError / ValueError -- nothing has been launched yet -- returns
    {'error': message}.  ``band_report`` (True, a number of rings or (lo, hi) pairs; bands.report_bounds): the result
    also carries 'bands', the error by radius of the validation with the best PSNR.  config['ring_normalization'] (a
    config value or a searched one): the result carries the trial's table; the trainer scales into a buffer of its own, so
    the cached dataset tensors ``data`` holds are the same bits after the trial as before it."""
    import torch
    cfg = trial_config(config, max_epoch)
    t0 = time.time()
    try:
        tr = build_trial_trainer(cfg, data, seed, device)
    except (NotImplementedError, ValueError) as e:
        return {"error": "{}: {}".format(type(e).__name__, e)}
    prefix = "config_{}_".format(cfg.get("config_index", 0))
    on_validate = None
    if band_report is not None:
        tr.enable_band_report(None if band_report is True else band_report)
    if image_directory is not None:
        tr.enable_validation_images()
        if not os.path.exists(os.path.join(image_directory, "train.png")):  # hp_model_training.py:30-38, once
            tr.save_training_images(image_directory)

        def on_validate(rec):
            tr.save_validation_images(rec["epoch"], rec, image_directory, prefix=prefix)
    torch.cuda.synchronize()
    t1 = time.time()
    print("Training for {} epochs".format(max_epoch))
    tr.fit(val_epoch=cfg["val_epoch"], on_validate=on_validate)
    torch.cuda.synchronize()
    t2 = time.time()
    stats = dict(INITIAL_STATS)
    if tr.val_history:
        stats = {"best_psnr": tr.best_psnr, "best_psnr_ep": tr.best_psnr_ep, "best_ssim": tr.best_ssim,
                 "best_ssim_ep": tr.best_ssim_ep}
        print(tr.validation_line(tr.val_history[-1], max_epoch))
        if band_report is not None:  # the record of the epoch best_psnr names
            best = next((r for r in tr.val_history if r["epoch"] == tr.best_psnr_ep), tr.val_history[-1])
            stats.update({k: v for k, v in best.items() if k.startswith("bands")})
    else:
        print("hp search: config #{}: no validation epoch within max_epoch={} (val_epoch={}): its record keeps the "
              "initial {} / {}".format(cfg.get("config_index", 0), max_epoch, cfg["val_epoch"],
                                      INITIAL_STATS["best_psnr"], INITIAL_STATS["best_ssim"]))
    if tr.ring_table is not None:  # config['ring_normalization'], given or searched: the table this trial fitted under
        stats["ring_normalization"] = tr.ring_table.summary()
    return dict(stats, steps=tr.global_step, fit_seconds=t2 - t1, build_seconds=t1 - t0)


class LocalRunner:
    """Trials in this process: one DataCache, one library handle, for as long as the object lives."""

    def __init__(self, source: Callable, max_epoch: int, *, seed: int = 0, image_directory: Optional[str] = None,
                 device="cuda", cache_bytes: int = CACHE_BUDGET_BYTES, extra_key: tuple = (), run_trial=None,
                 band_report=None):
        self.cache = DataCache(source, cache_bytes, device if run_trial is None else None, extra_key)
        self.max_epoch, self.seed, self.image_directory, self.device = max_epoch, seed, image_directory, device
        self.run_trial, self.band_report = run_trial, band_report

    def __call__(self, merged: dict) -> dict:
        t0 = time.time()
        data = self.cache.get(merged)
        ingest = time.time() - t0
        if self.run_trial is not None:
            res = dict(self.run_trial(merged, self.max_epoch, data))
        else:
            res = hp_training_function(merged, self.max_epoch, data, seed=self.seed,
                                       image_directory=self.image_directory, device=self.device,
                                       band_report=self.band_report)
        res["setup_seconds"] = ingest + res.pop("build_seconds", 0.0)
        return res


def is_trial_result(res) -> bool:
    """A result (the four statistics) or a recorded refusal ({'error': message})."""
    if not isinstance(res, dict):
        return False
    if "error" in res:
        return isinstance(res["error"], str)
    return all(isinstance(res.get(k), (int, float)) and not isinstance(res.get(k), bool) for k in STAT_KEYS)


# ---- worker processes -------------------------------------------------------------------------------------------------
# Protocol, one JSON object per line.  Parent -> child stdin: first {"setup": {...}}, then {"trial": i, "config": merged}
# one at a time; the child answers each trial with {"trial": i, "result": {...}} on its stdout and exits 0 when its stdin
# closes.  Everything else a worker prints goes to its stderr, which is the parent's.
def worker_main() -> int:
    proto = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)  # the library's and the trainers' prints must not land between protocol lines
    sys.stdout = sys.stderr
    setup = json.loads(sys.stdin.readline())["setup"]
    syn = setup.get("synthetic")
    source = synthetic_source(*syn) if syn else dataset_source
    runner = LocalRunner(source, setup["max_epoch"], seed=setup["seed"], image_directory=setup.get("image_directory"),
                         cache_bytes=setup.get("cache_bytes", CACHE_BUDGET_BYTES), extra_key=tuple(syn or ()),
                         band_report=setup.get("band_report"))
    for line in sys.stdin:
        if not line.strip():
            continue
        msg = json.loads(line)
        res = runner(msg["config"])
        res["ingests"] = runner.cache.ingests
        proto.write(json.dumps({"trial": msg["trial"], "result": res}) + "\n")
        proto.flush()
    return 0


class _Worker:
    def __init__(self, index: int, cmd: list, setup: dict):
        self.index = index
        self.proc = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, env=_child_env())
        self.buf = b""
        self.trial = None  # index of the trial it is running
        self.deadline = None
        self.ingests = 0
        try:
            self.send({"setup": setup})
        except OSError:  # gone already: the first read sees the end of its output
            pass

    def send(self, msg: dict) -> None:
        self.proc.stdin.write((json.dumps(msg) + "\n").encode())
        self.proc.stdin.flush()

    def kill(self) -> None:
        if self.proc.poll() is None:
            self.proc.kill()
        self.proc.wait()


def _child_env() -> dict:
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.environ.get("PYTHONPATH")
    return dict(os.environ, PYTHONPATH=pkg + (os.pathsep + path if path else ""))


def run_workers(merged: list, jobs: int, setup: dict, records: dict, *, trial_timeout: float = TRIAL_TIMEOUT,
                worker_cmd: Optional[list] = None) -> dict:
    """Runs the trials ``merged`` on ``jobs`` fresh child processes, one trial per child at a time, filling
    ``records[i] = result`` (plus 'worker').  Failure rule: a child that exits non-zero, dies on a signal, runs a trial
    past ``trial_timeout`` seconds (it is killed) or answers anything but a result / recorded refusal for the trial it
    was given stops the dispatch: no further trial is handed out, the other running trials finish, nothing is retried.
    Returns {'aborted': None or the reason, 'ingests': source calls over all workers}."""
    cmd = list(worker_cmd or WORKER_CMD)
    workers, aborted, nxt = [], None, 0
    try:
        for w in range(min(jobs, len(merged))):
            workers.append(_Worker(w, cmd, setup))
        live = list(workers)
        while True:
            for w in live:
                if aborted is None and w.trial is None and nxt < len(merged):
                    print("\nEvaluating Config #{} [of {}] on worker {}".format(nxt + 1, len(merged), w.index), flush=True)
                    try:
                        w.send({"trial": nxt, "config": merged[nxt]})
                    except OSError:  # it has gone already: the read below sees the end of its output
                        pass
                    w.trial, w.deadline = nxt, time.time() + trial_timeout
                    nxt += 1
            busy = [w for w in live if w.trial is not None]
            if not busy:
                break
            wait = max(0.0, min(w.deadline for w in busy) - time.time())
            ready, _, _ = select.select([w.proc.stdout for w in busy], [], [], wait)
            for w in busy:
                failure = None
                if w.proc.stdout in ready:
                    chunk = os.read(w.proc.stdout.fileno(), 1 << 16)
                    if not chunk:
                        w.proc.wait()
                        failure = "worker {} ended with status {} during trial {}".format(w.index, w.proc.returncode,
                                                                                          w.trial + 1)
                    w.buf += chunk
                    while failure is None and b"\n" in w.buf:
                        line, w.buf = w.buf.split(b"\n", 1)
                        try:
                            msg = json.loads(line)
                        except ValueError:
                            msg = None
                        if not (isinstance(msg, dict) and msg.get("trial") == w.trial
                                and is_trial_result(msg.get("result"))):
                            failure = "worker {} answered trial {} with {!r}".format(w.index, (w.trial or 0) + 1,
                                                                                     line[:200])
                            break
                        res = msg["result"]
                        w.ingests = res.pop("ingests", w.ingests)
                        records[w.trial] = dict(res, worker=w.index)
                        w.trial = w.deadline = None
                elif time.time() >= w.deadline:
                    failure = "worker {} ran trial {} past {:g} s".format(w.index, w.trial + 1, trial_timeout)
                if failure is not None:
                    w.kill()
                    w.trial = None
                    live.remove(w)
                    aborted = aborted or failure
                    print("hp search: " + failure + ": no further trial is started", file=sys.stderr, flush=True)
        for w in live:  # end of input is the workers' signal to leave; a non-zero exit counts even now
            w.proc.stdin.close()
        for w in live:
            try:
                rc = w.proc.wait(timeout=60)
            except subprocess.TimeoutExpired:
                rc = "a timeout"
            if rc != 0:
                aborted = aborted or "worker {} ended with status {}".format(w.index, rc)
    finally:
        for w in workers:
            w.kill()
    return {"aborted": aborted, "ingests": sum(w.ingests for w in workers)}


# ---- the search (find_best_config.py:28-95, hp_search_script.py:59-67) ------------------------------------------------
def _json_value(v):
    return v if isinstance(v, (int, float, str, bool, type(None), list, dict)) else repr(v)


def write_results(output_directory: str, hp_configs: list, records: dict, aborted) -> list:
    rows = []
    for i in sorted(records):
        rows.append(dict({"index": i + 1, "hp": {k: _json_value(v) for k, v in hp_configs[i].items()}}, **records[i]))
    with open(os.path.join(output_directory, "results.json"), "w") as f:
        json.dump({"aborted": bool(aborted), "reason": aborted or None, "trials": len(hp_configs), "results": rows}, f,
                  indent=1)
    return rows


def run_search(config: dict, hp_config: dict, output_directory: str, *, source: Optional[Callable] = None,
               seed: int = 0, search_seed: Optional[int] = None, jobs: int = 1, save_images: bool = False,
               run_trial: Optional[Callable] = None, synthetic: Optional[tuple] = None,
               trial_timeout: float = TRIAL_TIMEOUT, cache_bytes: int = CACHE_BUDGET_BYTES,
               worker_cmd: Optional[list] = None, band_report=None) -> dict:
    """hp_search_script.py:12-67 into ``output_directory`` (which exists): hp_search_config_{i}.yaml per trial,
    best_psnr_config.yaml, best_ssim_config.yaml, configs_and_results.txt, results.json; pictures in
    <output_directory>/images with ``save_images``; with ``band_report`` (True or a number of rings) every trial's record
    in results.json carries 'bands', the error by radius of its best validation.

    ``source``: cfg -> (image, coords, shape), called once per distinct dataset (default: the scan the config names, or
    make_kspace of ``synthetic`` = (C, H, W)).  ``run_trial(merged_config, max_epoch, data) -> dict`` replaces the
    trainer fit (host logic on the CPU).  ``jobs`` > 1: that many worker processes (at most MAX_JOBS), which build the
    default source themselves -- a ``source`` / ``run_trial`` callable cannot cross into them; ``trial_timeout`` is the
    time one of THEM may spend on a trial (with jobs == 1 the trials run in this process and nothing limits them).
    Returns {'results',
    'best_psnr', 'best_ssim' (each {'index', 'value', 'config'} or None), 'ingests', 'aborted', 'output_directory'}."""
    from .train import set_default_configs
    jobs = int(jobs)
    if not 1 <= jobs <= MAX_JOBS:
        raise ValueError(f"jobs={jobs}: 1..{MAX_JOBS} (the GPU boxes are shared and allow 16 GPU processes in total)")
    if jobs > 1 and (source is not None or run_trial is not None):
        raise ValueError("jobs > 1 runs trials in fresh processes: they cannot take a source / run_trial callable")
    config = set_default_configs(copy.deepcopy(config))
    hp_config = copy.deepcopy(hp_config)
    check_search(config, hp_config)
    max_epoch = int(hp_config["max_epoch"])
    print("** Running {} Search **".format("Grid" if hp_config["method"] == "grid" else "Random"))
    hp_configs = expand_trials(hp_config, search_seed)  # all sampling here, in the parent: the list ignores ``jobs``
    merged = merged_configs(config, hp_configs)
    image_directory = None
    if save_images:
        image_directory = os.path.join(output_directory, "images")
        os.makedirs(image_directory, exist_ok=True)
    for i, hp in enumerate(hp_configs):  # find_best_config.py:53-54
        with open(os.path.join(output_directory, "hp_search_config_{}.yaml".format(i + 1)), "w") as f:
            yaml.dump(hp, f, default_flow_style=False)

    records, aborted, ingests = {}, None, 0
    if jobs == 1:
        if source is None:
            source = synthetic_source(*synthetic) if synthetic else dataset_source
        runner = LocalRunner(source, max_epoch, seed=seed, image_directory=image_directory, cache_bytes=cache_bytes,
                             extra_key=tuple(synthetic or ()), run_trial=run_trial, band_report=band_report)
        try:
            for i, cfg in enumerate(merged):
                print("\nEvaluating Config #{} [of {}]:\n".format(i + 1, len(hp_configs)), hp_configs[i])
                res = runner(cfg)
                if not is_trial_result(res):
                    raise RuntimeError("hp search: trial {} returned {!r}".format(i + 1, res))
                records[i] = dict(res, worker=0)
        except BaseException as e:  # any other failure ends the search at once; what there is gets written
            write_results(output_directory, hp_configs, records, "{}: {}".format(type(e).__name__, e))
            raise
        ingests = runner.cache.ingests
    else:
        setup = {"max_epoch": max_epoch, "seed": seed, "image_directory": image_directory,
                 "synthetic": list(synthetic) if synthetic else None, "cache_bytes": cache_bytes,
                 "band_report": band_report}
        out = run_workers(merged, jobs, setup, records, trial_timeout=trial_timeout, worker_cmd=worker_cmd)
        aborted, ingests = out["aborted"], out["ingests"]

    # find_best_config.py:78-86, strict '>' from the reference's initial values: ties keep the earlier trial; a recorded
    # refusal has no statistics and never wins.  The winners are copies of THEIR configs (the reference aliases the dict
    # it keeps mutating, so both of its files hold the last trial's).
    best = {"psnr": (INITIAL_STATS["best_psnr"], None), "ssim": (INITIAL_STATS["best_ssim"], None)}
    for i in sorted(records):
        if "error" in records[i]:
            continue
        for m in best:
            if records[i]["best_" + m] > best[m][0]:
                best[m] = (records[i]["best_" + m], i)
    rows = write_results(output_directory, hp_configs, records, aborted)
    result = {"results": rows, "ingests": ingests, "aborted": bool(aborted), "reason": aborted,
              "output_directory": output_directory}
    for m, (value, i) in best.items():
        won = None if i is None else {"index": i + 1, "value": value, "config": copy.deepcopy(merged[i])}
        result["best_" + m] = won
        print("\nSearch done. Best {} = {}".format("Psnr" if m == "psnr" else "SSIM", value))
        print("Best Config {}:".format(m.upper()), None if won is None else won["config"])
        with open(os.path.join(output_directory, "best_{}_config.yaml".format(m)), "w") as f:
            yaml.dump(None if won is None else won["config"], f, default_flow_style=False)
    with open(os.path.join(output_directory, "configs_and_results.txt"), "w") as f:
        for i in sorted(records):
            stats = {k: v for k, v in records[i].items() if k in STAT_KEYS + ("error",)}
            f.write("{} -> {}\n".format(hp_configs[i], stats))
    return result


def search_directory(config: dict, hp_config: dict, config_path: str, output_path: str) -> str:
    """hp_search_script.py:24-35: <output_path>/outputs/<model_name><timestamp>."""
    output_folder = os.path.splitext(os.path.basename(config_path))[0]
    model_name = os.path.join(output_folder, str(config.get("data", "synthetic")) + "/img_{}_{}_{}_{}_{}_lr{:.2g}_encoder_{}_hp_{}_search_"
                              .format(config["model"], config["net"]["network_input_size"],
                                      config["net"]["network_width"], config["net"]["network_depth"], config["loss"],
                                      config["lr"], config["encoder"]["embedding"], hp_config["method"]))
    if not (config["encoder"]["embedding"] == "none"):
        model_name += "_scale{}_size{}".format(config["encoder"]["scale"], config["encoder"]["embedding_size"])
    return os.path.join(output_path + "/outputs", model_name + datetime.now().strftime("%Y-%m-%d_%H-%M-%S"))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description="grid / random hyperparameter search (hp_search_script.py)")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--config", type=str, help="Path to the config file.")
    ap.add_argument("--hp_config", type=str, help="Path to the HP config file (YAML or the reference's JSON).")
    ap.add_argument("--output_path", type=str, default=".", help="outputs path")
    ap.add_argument("--synthetic", type=str, default=None,
                    help="C,H,W: search on a synthetic k-space of that shape instead of the scan the config names")
    ap.add_argument("--seed", type=int, default=0, help="seed of every trial's encoder (the model is seeded with 42)")
    ap.add_argument("--search-seed", type=int, default=None, help="random.seed() before sampling (default: unseeded)")
    ap.add_argument("--jobs", type=int, default=1, help="worker processes running trials side by side (1..%d)" % MAX_JOBS)
    ap.add_argument("--save-images", action="store_true", help="write every trial's validation pictures to <dir>/images")
    ap.add_argument("--trial-timeout", type=float, default=TRIAL_TIMEOUT,
                    help="with --jobs > 1: seconds a worker process may spend on one trial before it is killed and the "
                         "search stops (with --jobs 1 trials run in this process and are not limited)")
    ap.add_argument("--cache-bytes", type=int, default=CACHE_BUDGET_BYTES,
                    help="bytes of resident datasets kept between trials (0: ingest for every trial)")
    from .bands import add_band_report_flag, flag_bounds
    add_band_report_flag(ap, "per trial")
    from .coils import add_virtual_coils_flag, apply_virtual_coils_flag
    add_virtual_coils_flag(ap)
    opts = ap.parse_args(argv)
    if opts.worker:
        return worker_main()
    if not opts.config or not opts.hp_config:
        ap.error("--config and --hp_config are required")
    if not 1 <= opts.jobs <= MAX_JOBS:
        ap.error("--jobs {}: 1..{} (the GPU boxes are shared and allow 16 GPU processes in total)".format(opts.jobs, MAX_JOBS))
    from .train import get_config, set_default_configs
    config = apply_virtual_coils_flag(set_default_configs(get_config(opts.config)), opts)
    hp_config = get_config(opts.hp_config)
    check_search(config, hp_config)
    output_directory = search_directory(config, hp_config, opts.config, opts.output_path)
    os.makedirs(output_directory, exist_ok=True)
    import shutil
    shutil.copy(opts.config, os.path.join(output_directory, "config.yaml"))  # hp_search_script.py:37
    res = run_search(config, hp_config, output_directory, seed=opts.seed, search_seed=opts.search_seed, jobs=opts.jobs,
                     save_images=opts.save_images, band_report=flag_bounds(opts.band_report),
                     trial_timeout=opts.trial_timeout, cache_bytes=opts.cache_bytes,
                     synthetic=tuple(int(v) for v in opts.synthetic.split(",")) if opts.synthetic else None)
    print(json.dumps({"output_directory": output_directory, "trials": len(res["results"]), "ingests": res["ingests"],
                      "aborted": res["aborted"],
                      "best_psnr": res["best_psnr"] and {k: res["best_psnr"][k] for k in ("index", "value")},
                      "best_ssim": res["best_ssim"] and {k: res["best_ssim"][k] for k in ("index", "value")}}))
    return 1 if res["aborted"] else 0


if __name__ == "__main__":
    sys.exit(main())
