"""checkpoint.py's part functions on the host (no GPU, no library): the layout of the joined 'opt' against a real
torch.optim.Adam over the chained parameters, the round trip through load_parts, what a shifted boundary does, and the
joined 'net' against the three trainers' join functions as they stood before they shared one (restated below)."""
import itertools
from collections import OrderedDict

import pytest
import torch

from inr_mi355x import checkpoint as CK
from inr_mi355x.networks import FFN, SIREN, WIRE

CONFIG = dict(lr=1e-3, beta1=0.9, beta2=0.999, weight_decay=0.0)
NET = dict(network_input_size=6, network_output_size=2, network_depth=3, network_width=8)


class StubEngine:
    """what optimizer_state / load_dict touch of an engine: flat CPU moments over the model's layout and a step count"""

    def __init__(self, model, step, seed=None):
        n = model._flat.numel()
        if seed is None:
            self.exp_avg, self.exp_avg_sq = torch.zeros(n), torch.zeros(n)
        else:
            g = torch.Generator().manual_seed(seed)
            self.exp_avg, self.exp_avg_sq = torch.randn(n, generator=g), torch.rand(n, generator=g)
        self.step = step
        self.packs = 0

    def pack(self):
        self.packs += 1


def _models(n):
    torch.manual_seed(0)
    wire = dict(NET, network_width=12, first_omega_0=10.0, hidden_omega_0=10.0, scale=10.0)
    return [cls(p) for cls, p in zip((SIREN, FFN, WIRE), (NET, NET, wire))][:n]


def _parts(models, steps, seeded=True):
    return [CK.Part(f"p{k}.", m, StubEngine(m, s, seed=10 + k if seeded else None))
            for k, (m, s) in enumerate(zip(models, steps))]


def _stateful_positions(parts):
    """positions in the chained parameters() of the parameters that carry Adam state"""
    chained = list(itertools.chain(*[p.model.parameters() for p in parts]))
    have = {id(q) for p in parts if p.engine.step for q, lv in
            zip(p.model._flat_params, getattr(p.model, "_live", [True] * len(p.model._flat_params))) if lv}
    return [j for j, q in enumerate(chained) if id(q) in have], chained


@pytest.mark.parametrize("n", [1, 2, 3])
def test_joined_optimizer_state_is_one_adam_over_the_chained_parameters(n):
    parts = _parts(_models(n), [5] * n)
    opt = CK.joined_optimizer_state(parts, CONFIG)
    want, chained = _stateful_positions(parts)
    assert sorted(opt["state"]) == want
    assert len(want) < len(chained) or n < 3  # WIRE's frozen omega_0 / scale_0 are parameters without state
    single = CK.optimizer_state(parts[0].model, parts[0].engine, CONFIG)["param_groups"][0]
    assert len(opt["param_groups"]) == 1
    group = opt["param_groups"][0]
    assert group["params"] == list(range(len(chained)))
    assert {k: v for k, v in group.items() if k != "params"} == {k: v for k, v in single.items() if k != "params"}
    adam = torch.optim.Adam(chained, lr=CONFIG["lr"])
    adam.load_state_dict(opt)
    for j in want:
        assert torch.equal(adam.state[chained[j]]["exp_avg"], opt["state"][j]["exp_avg"])
        assert adam.state[chained[j]]["exp_avg"].shape == chained[j].shape


@pytest.mark.parametrize("steps", [(5,), (5, 5), (5, 5, 5), (5, 0, 5)], ids=str)
def test_load_parts_round_trip(steps):
    """every moment tensor and every step count come back; a part at step 0 wrote no state and loads as zeros"""
    src = _parts(_models(len(steps)), steps)
    opt = CK.joined_optimizer_state(src, CONFIG)
    nets = [p.model.state_dict() for p in src]
    dst = _parts(_models(len(steps)), [9] * len(steps))  # other moments, another step: all of it is overwritten
    CK.load_parts(dst, nets, [None] * len(steps), opt)
    for s, d in zip(src, dst):
        assert d.engine.step == s.engine.step and d.engine.packs == 1
        live = getattr(s.model, "_live", [True] * len(s.model._layout))
        for (off, n, _, _), lv in zip(s.model._layout, live):
            for name in ("exp_avg", "exp_avg_sq"):
                want = getattr(s.engine, name)[off:off + n] if s.engine.step and lv else torch.zeros(n)
                assert torch.equal(getattr(d.engine, name)[off:off + n], want), name
        assert torch.equal(d.model._flat, s.model._flat)
    # without 'opt' every part loads as zeros at step 0; weights_only leaves the optimizer state alone
    CK.load_parts(dst, nets, [None] * len(steps), None)
    assert all(d.engine.step == 0 and not d.engine.exp_avg.any() for d in dst)
    kept = _parts(_models(len(steps)), [9] * len(steps))
    before = [k.engine.exp_avg.clone() for k in kept]
    CK.load_parts(kept, nets, [None] * len(steps), None, weights_only=True)
    assert all(k.engine.step == 9 and k.engine.packs == 1 and torch.equal(k.engine.exp_avg, b) for k, b in zip(kept, before))


def test_a_shifted_boundary_does_not_load_silently(monkeypatch):
    """The 'opt' of a checkpoint whose first part had ONE parameter more than the loader's: the joined state of matching
    parts with one entry put in at index n0 and everything behind it moved up by one.  Cut by the loader's counts, part 0
    loads clean (its own entries are where they were) and part 1 is offered the extra entry for its first parameter and,
    from there on, every moment of the parameter before.  What then happens is a matter of shapes, because copy_
    broadcasts: the extra entry, (6,), goes into the (8, 6) weight without a word; the weight's own (8, 6) moments,
    offered to the (8,) bias next, do not fit, and load_dict raises there -- in part 1, after part 0 was loaded."""
    theirs = _parts(_models(2), (5, 5))
    mine = _parts(_models(2), (0, 0), seeded=False)
    opt = CK.joined_optimizer_state(theirs, CONFIG)
    n0 = len(list(mine[0].model.parameters()))
    extra = {"step": torch.tensor(5.0), "exp_avg": torch.full((6,), 7.0), "exp_avg_sq": torch.full((6,), 7.0)}
    state = {j if j < n0 else j + 1: st for j, st in opt["state"].items()}
    state[n0] = extra
    shapes = [tuple(p.shape) for p in mine[1].model.parameters()][:2]
    assert shapes == [(8, 6), (8,)] and tuple(state[n0 + 1]["exp_avg"].shape) == (8, 6)
    entered = []
    real = CK.load_dict
    monkeypatch.setattr(CK, "load_dict", lambda model, *a, **kw: (entered.append(model), real(model, *a, **kw))[1])
    with pytest.raises(RuntimeError, match="size of tensor"):
        CK.load_parts(mine, [p.model.state_dict() for p in mine], [None, None], {"state": state})
    assert entered == [mine[0].model, mine[1].model]  # part 0 went through; the objection is part 1's
    assert mine[0].engine.step == 5 and torch.equal(mine[0].engine.exp_avg, theirs[0].engine.exp_avg)
    off, n, _, _ = mine[1].model._layout[0]
    assert bool((mine[1].engine.exp_avg[off:off + n] == 7.0).all())  # the broadcast copy that nothing refused


def test_load_parts_refuses_lists_of_different_lengths():
    parts = _parts(_models(2), (0, 0))
    nets = [p.model.state_dict() for p in parts]
    for bad_nets, bad_encs in ((nets[:1], [None, None]), (nets, [None]), (nets + nets[:1], [None, None])):
        with pytest.raises(ValueError, match="2 parts"):
            CK.load_parts(parts, bad_nets, bad_encs, None)


# ---- the three join functions as they were written out per trainer ------------------------------------------------------
def _old_wrapper_state(backbone, scaler):
    net = OrderedDict()
    for prefix, mod in (("backbone.", backbone), ("scaler.", scaler)):
        for k, v in mod.state_dict().items():
            net[prefix + k] = v.detach().clone()
    return net


def _old_merge_state(experts, gate):
    net = OrderedDict()
    for k, sd in enumerate(experts):
        for name, v in sd.items():
            net[f"heads.{k}.{name}"] = v.detach().clone()
    for name, v in gate.items():
        net["weighted_avg." + name] = v.detach().clone()
    return net


def _old_join_state(image_state, sens_state):
    net = OrderedDict()
    for prefix, sd in (("image.", image_state), ("sens.", sens_state)):
        for k, v in sd.items():
            net[prefix + k] = v.detach().clone()
    return net


def _same(got, want):
    assert list(got) == list(want)
    for k in want:
        assert torch.equal(got[k], want[k]) and got[k].data_ptr() != want[k].data_ptr(), k


def test_joined_net_gives_the_three_trainers_keys_in_order():
    from inr_mi355x import sense, train_multihead, train_scaling
    a, b, c = _models(3)
    P = lambda prefix, m: CK.Part(prefix, m, None)
    _same(CK.joined_net([P("backbone.", a), P("scaler.", b)]), _old_wrapper_state(a, b))
    _same(train_scaling.wrapper_state(a, b), _old_wrapper_state(a, b))
    old = _old_merge_state([a.state_dict(), c.state_dict()], b.state_dict())
    _same(CK.joined_net([P("heads.0.", a), P("heads.1.", c), P("weighted_avg.", b)]), old)
    _same(train_multihead.merge_state([a.state_dict(), c.state_dict()], b.state_dict()), old)
    _same(CK.joined_net([P("image.", a), P("sens.", b)]), _old_join_state(a.state_dict(), b.state_dict()))
    _same(sense.join_state(a.state_dict(), b.state_dict()), _old_join_state(a.state_dict(), b.state_dict()))
    _same(CK.joined_net([P("image.", a)]), OrderedDict(("image." + k, v) for k, v in a.state_dict().items()))
    for split, joined in ((train_scaling.split_state, _old_wrapper_state(a, b)),
                          (sense.split_state, _old_join_state(a.state_dict(), b.state_dict()))):
        x, y = split(joined)
        assert list(x) == list(a.state_dict()) and list(y) == list(b.state_dict())
    heads, gate = train_multihead.split_state(old)
    assert [list(h) for h in heads] == [list(a.state_dict()), list(c.state_dict())] and list(gate) == list(b.state_dict())


def test_foreign_keys_are_refused_with_the_trainers_messages():
    from inr_mi355x import sense, train_multihead, train_scaling
    a, b, _ = _models(3)
    with pytest.raises(ValueError, match=r"keys outside 'backbone\.' / 'scaler\.': \['other\.w'\]"):
        train_scaling.split_state(dict(_old_wrapper_state(a, b), **{"other.w": torch.zeros(1)}))
    with pytest.raises(ValueError, match=r"keys outside 'image\.' / 'sens\.': \['other\.w'\]"):
        sense.split_state(dict(_old_join_state(a.state_dict(), b.state_dict()), **{"other.w": torch.zeros(1)}))
    with pytest.raises(ValueError, match=r"a SENSE checkpoint holds both 'image\.' and 'sens\.' keys"):
        sense.split_state({"image." + k: v for k, v in a.state_dict().items()})
    with pytest.raises(ValueError, match=r"key 'other\.w' outside 'heads\.' / 'weighted_avg\.'"):
        train_multihead.split_state({"other.w": torch.zeros(1)})
    with pytest.raises(ValueError, match=r"key 'heads\.x\.w': expected 'heads\.<k>\.<parameter>'"):
        train_multihead.split_state({"heads.x.w": torch.zeros(1)})
