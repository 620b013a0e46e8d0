"""Checkpoint interchange with the reference: the dict ``{'net', 'enc', 'opt'}`` of train.py:247-250 /
train_kspace_multiscale.py, with ``'opt'`` in ``torch.optim.Adam.state_dict()`` layout (state indexed by the
position of the parameter in ``model.parameters()``; frozen / never-stepped parameters have no entry), and the
``config["pretrain"]`` resume path of train.py:117-121.
"""
from collections import OrderedDict
from typing import Callable, NamedTuple, Optional, Sequence

import torch

from .networks import _view


def _param_positions(model):
    """position in model.parameters() of every flat-buffer parameter, in layout order."""
    pos = {id(p): j for j, p in enumerate(model.parameters())}
    return [pos[id(p)] for p in model._flat_params]


def optimizer_state(model, engine, config: dict) -> dict:
    live = getattr(model, "_live", [True] * len(model._layout))
    state = {}
    for (off, n, shp, cplx), j, lv in zip(model._layout, _param_positions(model), live):
        if engine.step == 0 or not lv:
            continue  # Adam creates state lazily at the first step with a gradient
        state[j] = {"step": torch.tensor(float(engine.step)),
                    "exp_avg": _view(engine.exp_avg, off, n, shp, cplx).clone(),
                    "exp_avg_sq": _view(engine.exp_avg_sq, off, n, shp, cplx).clone()}
    n_params = len(list(model.parameters()))
    group = {"lr": config["lr"], "betas": (config["beta1"], config["beta2"]), "eps": 1e-8,
             "weight_decay": config["weight_decay"], "amsgrad": False, "maximize": False, "foreach": None,
             "capturable": False, "differentiable": False, "fused": None, "params": list(range(n_params))}
    return {"state": state, "param_groups": [group]}


class Part(NamedTuple):
    """One network of a fit that drives several under one Adam: its key prefix in 'net', the model, its engine, the
    encoder that travels with it (or None) and what to call when a checkpoint replaced that encoder's matrix."""
    prefix: str
    model: object
    engine: object
    encoder: object = None
    rebind: Optional[Callable] = None


def joined_net(parts: Sequence[Part]) -> OrderedDict:
    """'net' of several networks: prefix + key of every part's state_dict, in part order (clones: a checkpoint must not
    alias the running weights)"""
    return OrderedDict((p.prefix + k, v.detach().clone()) for p in parts for k, v in p.model.state_dict().items())


def joined_optimizer_state(parts: Sequence[Part], config: dict) -> dict:
    """'opt' of ONE Adam over the parts' parameters in part order: every part's optimizer_state with its indices moved
    behind the parameters of the parts in front of it, and one param group over all of them."""
    opt, base = None, 0
    for p in parts:
        part = optimizer_state(p.model, p.engine, config)
        if opt is None:
            opt = part
        else:
            opt["state"].update({j + base: st for j, st in part["state"].items()})
        base += len(part["param_groups"][0]["params"])
    opt["param_groups"][0]["params"] = list(range(base))
    return opt


def split_prefixed(net_state: dict, prefixes: Sequence[str]) -> list:
    """[state_dict per prefix] of a joined 'net', the prefix cut off; ValueError for keys under none of them"""
    other = [k for k in net_state if not k.startswith(tuple(prefixes))]
    if other:
        raise ValueError(f"keys outside {' / '.join(repr(p) for p in prefixes)}: {other[:4]}")
    return [OrderedDict((k[len(p):], v) for k, v in net_state.items() if k.startswith(p)) for p in prefixes]


def load_parts(parts: Sequence[Part], nets: Sequence[dict], encs: Sequence, opt: Optional[dict],
               weights_only: bool = False) -> None:
    """The inverse of joined_net / joined_optimizer_state: ``nets`` the parts' state_dicts (already split), ``encs`` the
    encoder matrix that goes with each (None: none), ``opt`` the joined 'opt', cut by the running count of
    model.parameters().  ``weights_only``: load_weights and a re-pack, no optimizer state (a reconstruction's path)."""
    if not len(parts) == len(nets) == len(encs):
        raise ValueError(f"{len(parts)} parts, {len(nets)} state dicts and {len(encs)} encoder matrices")
    base = 0
    for p, net, enc in zip(parts, nets, encs):
        n = len(list(p.model.parameters()))
        if weights_only:
            load_weights(p.model, p.encoder, {"net": net, "enc": enc}, p.rebind)
            p.engine.pack()
        else:
            sub = {"state": {j - base: st for j, st in opt["state"].items() if base <= j < base + n}} if opt else None
            load_dict(p.model, p.encoder, p.engine, {"net": net, "enc": enc, "opt": sub}, p.rebind)
        base += n


def save_dict(model, encoder, engine, config: dict) -> dict:
    # clones: the live state_dict entries are views of ONE flat buffer (float and complex views of the same storage
    # cannot be pickled together, and a checkpoint must not alias the running weights)
    net = type(model.state_dict())((k, v.detach().clone()) for k, v in model.state_dict().items())
    return {"net": net, "enc": None if encoder.B is None else encoder.B.clone(),
            "opt": optimizer_state(model, engine, config)}


@torch.no_grad()
def load_weights(model, encoder, ckpt: dict, rebind=None) -> None:
    """model.load_state_dict(ckpt['net']); encoder.B = ckpt['enc'].  No optimizer state is read or touched: what a
    reconstruction needs of a checkpoint.  The caller re-packs its engine."""
    model.load_state_dict(ckpt["net"])
    if ckpt.get("enc") is not None and encoder is not None:
        encoder.B = ckpt["enc"].to(encoder.B.device if encoder.B is not None else ckpt["enc"].device)
        if rebind is not None:
            rebind(encoder)  # the fused kernels hold their own contiguous copy of B


@torch.no_grad()
def load_dict(model, encoder, engine, ckpt: dict, rebind=None) -> None:
    """model.load_state_dict(ckpt['net']); optim.load_state_dict(ckpt['opt']); encoder.B = ckpt['enc']."""
    load_weights(model, encoder, ckpt, rebind)
    opt: Optional[dict] = ckpt.get("opt")
    engine.exp_avg.zero_()
    engine.exp_avg_sq.zero_()
    engine.step = 0
    if opt:
        steps = set()
        for (off, n, shp, cplx), j in zip(model._layout, _param_positions(model)):
            st = opt["state"].get(j)
            if st is None:
                continue
            _view(engine.exp_avg, off, n, shp, cplx).copy_(st["exp_avg"].to(engine.exp_avg.device))
            _view(engine.exp_avg_sq, off, n, shp, cplx).copy_(st["exp_avg_sq"].to(engine.exp_avg.device))
            steps.add(int(st["step"]))
        if len(steps) > 1:
            raise ValueError(f"parameters with different Adam step counts {sorted(steps)}: the engine keeps one")
        engine.step = steps.pop() if steps else 0
    engine.pack()
