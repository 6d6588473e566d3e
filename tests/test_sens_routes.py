"""Which C entry point each form of the per-step device calls reaches (QpalmBatch.step_device, active_device, adjoint_device, tangent_device,
adjoints_device, tangents_device, polish_device):

    no select, no at, no K            qpg_batch_<name>_device
    select only                       qpg_batch_<name>_subset_device
    at (with or without select)       qpg_batch_<name>_at_device
    the plural methods                qpg_batch_<name>_multi_device, whatever else is given

The name matters beyond the bits: it is the one the library's error messages carry.  The batch's `L` is replaced by a proxy that records the name of
every qpg_batch_* function called through it and forwards the call; nothing compiled is looked at.  The single and the plural methods share one
Python body: slice 0 of a plural call with K = 1 must hold the single call's bits (tests/test_sens_multi.py has the larger K).

Shape: the small batch of the refusal tests, B = 2 (n = 12, m = 20, five planted active rows), solved once per backend."""
import numpy as np
import torch

from tests.sens_helpers import T, point, small_batch


class Recorder:
    """forwards every attribute to the loaded library; the qpg_batch_* functions leave their names in `calls`"""

    def __init__(self, L):
        self._L, self.calls = L, []

    def __getattr__(self, name):
        fn = getattr(self._L, name)
        if not name.startswith("qpg_batch_"):
            return fn

        def recorded(*args):
            self.calls.append(name)
            return fn(*args)
        return recorded


_BATCH = {}


def recorded_batch(ctx):
    """(batch whose L records, its point (x, y, active), a select of member 0 alone)"""
    if ctx.kind not in _BATCH:
        bt, _ = small_batch(ctx, B=2)
        bt.solve()
        at = point(bt)
        bt.L = Recorder(bt.L)
        _BATCH[ctx.kind] = bt, at, T(ctx, [1, 0], np.int64)
    bt, at, sel = _BATCH[ctx.kind]
    assert bt.ctx is ctx
    return bt, at, sel


def names(bt, call):
    bt.L.calls.clear()
    out = call()
    return list(bt.L.calls), out


def test_every_form_calls_its_entry_point(ctx):
    bt, at, sel = recorded_batch(ctx)
    g1, g2 = T(ctx, np.ones((2, 12))), T(ctx, np.ones((2, 2, 12)))
    q = "qpg_batch_"
    # (entry point, select given?, the call)
    forms = [
        ("adjoint_device", False, lambda: bt.adjoint_device(g1)),
        ("adjoint_subset_device", True, lambda: bt.adjoint_device(g1, select=sel)),
        ("adjoint_at_device", False, lambda: bt.adjoint_device(g1, at=at)),
        ("adjoint_at_device", True, lambda: bt.adjoint_device(g1, at=at, select=sel)),
        ("tangent_device", False, lambda: bt.tangent_device(dq=g1)),
        ("tangent_subset_device", True, lambda: bt.tangent_device(dq=g1, select=sel)),
        ("tangent_at_device", False, lambda: bt.tangent_device(dq=g1, at=at)),
        ("tangent_at_device", True, lambda: bt.tangent_device(dq=g1, at=at, select=sel)),
        ("adjoint_multi_device", False, lambda: bt.adjoints_device(g2)),
        ("adjoint_multi_device", True, lambda: bt.adjoints_device(g2, select=sel)),
        ("adjoint_multi_device", False, lambda: bt.adjoints_device(g2, at=at)),
        ("tangent_multi_device", False, lambda: bt.tangents_device(dq=g2)),
        ("tangent_multi_device", True, lambda: bt.tangents_device(dq=g2, select=sel)),
        ("tangent_multi_device", False, lambda: bt.tangents_device(dq=g2, at=at)),
        ("polish_device", False, lambda: bt.polish_device()),
        ("polish_subset_device", True, lambda: bt.polish_device(select=sel)),
        ("get_active_device", None, lambda: bt.active_device()),
        ("get_active_subset_device", None, lambda: bt.active_device(select=sel)),
        # (the steps last: they move the batch on from the solve the point was recorded at)
        ("step_device", False, lambda: bt.step_device(warm="last")[1]),
        ("step_subset_device", True, lambda: bt.step_device(warm="last", select=sel)[1]),
    ]
    for i, (want, selects, call) in enumerate(forms):
        got, out = names(bt, call)
        assert got == [q + want], (i, got)
        if selects is not None:                                 # n_selected only when select was given: one member here
            assert ("n_selected" in out) == selects and out.get("n_selected", 1) == 1, (i, out.keys())
    assert bt.statuses().tolist() == [1, 1]


def test_a_plural_call_with_one_direction_is_the_single_call(ctx):
    bt, at, sel = recorded_batch(ctx)
    rng = np.random.default_rng(61)
    gx, gy = T(ctx, rng.standard_normal((2, 12))), T(ctx, rng.standard_normal((2, 20)))
    d = dict(dq=T(ctx, rng.standard_normal((2, 12))), dbmin=T(ctx, rng.standard_normal((2, 20))), dAx=T(ctx, rng.standard_normal((2, bt.nnzA))))
    rows = {False: slice(None), True: [0]}                      # with select only member 0's rows are written
    for kw in (dict(), dict(select=sel), dict(at=at), dict(at=at, select=sel)):
        got, one = names(bt, lambda: bt.adjoint_device(gx, gy, **kw))
        got_k, many = names(bt, lambda: bt.adjoints_device(gx[None], gy[None], **kw))
        assert got != got_k == ["qpg_batch_adjoint_multi_device"]
        got, one_t = names(bt, lambda: bt.tangent_device(**d, **kw))
        got_k, many_t = names(bt, lambda: bt.tangents_device(**{k: v[None] for k, v in d.items()}, **kw))
        assert got != got_k == ["qpg_batch_tangent_multi_device"]
        r = rows["select" in kw]
        for single, plural, keys in ((one, many, bt.ADJOINT_OUT), (one_t, many_t, bt.TANGENT_OUT)):
            assert set(single) == set(plural) == set(keys) | ({"n_selected"} if "select" in kw else set())
            for k in keys:
                first = plural[k] if k == "active" else plural[k][0]          # `active` is shared by the directions: no leading K
                assert first.shape == single[k].shape and first.dtype == single[k].dtype, (kw.keys(), k)
                assert torch.equal(first[r], single[k][r]), (kw.keys(), k)
            assert int(single["flag"][0]) == 0 and bool(single[keys[0]][0].abs().sum() > 0)
