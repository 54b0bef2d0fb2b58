"""Plan life cycles, the host side (no device): the LRU rule of ``UNetEngine._cached_plan`` over a plain dict, and the identity of a
training forward - ``TrainEngine.claim_forward`` / ``last_forward`` / ``holds_plan`` and what ``backward(forward=...)`` refuses -
on an engine that never saw a device, with empty ``TrainPlan`` objects standing in for built plans.  The sequences themselves run
in tests/test_gpu_plan_lifecycle.py."""
import pytest
import torch

from tests._common import SMALL, make_args
from worddiffusion_amd import UNetModel
from worddiffusion_amd.engine import UNetEngine
from worddiffusion_amd.train_engine import TrainPlan

cached = UNetEngine._cached_plan


def test_a_hit_becomes_the_most_recent_entry():
    plans = {"a": 1, "b": 2, "c": 3}
    assert cached(plans, "a", room=4) == 1
    assert list(plans) == ["b", "c", "a"] and plans == {"a": 1, "b": 2, "c": 3}
    assert cached(plans, "a", room=4) == 1 and list(plans) == ["b", "c", "a"]  # (already the most recent)
    assert cached(plans, "c") == 3 and list(plans) == ["b", "a", "c"]         # room = 0 reorders too
    # a hit never evicts, even in a dict that is over ``room``
    assert cached(plans, "b", room=1) == 2 and list(plans) == ["a", "c", "b"]


@pytest.mark.parametrize("room", [1, 2, 3, 4])
def test_a_miss_evicts_the_oldest_down_to_room_minus_one(room):
    plans = {k: k.upper() for k in "abcde"}
    assert cached(plans, "x", room=room) is None
    assert list(plans) == list("abcde")[6 - room:]  # the oldest went first
    assert len(plans) == room - 1 and "x" not in plans  # (the caller stores what it builds)
    plans["x"] = "X"
    assert len(plans) == room and list(plans)[-1] == "x"


def test_eviction_follows_use_not_insertion():
    plans = {"a": 1, "b": 2, "c": 3, "d": 4}
    cached(plans, "a", room=4)                 # a is now the most recent: b is the oldest
    assert cached(plans, "e", room=4) is None
    assert list(plans) == ["c", "d", "a"]


def test_room_zero_never_evicts():
    plans = {k: k for k in range(50)}
    assert cached(plans, "x") is None and cached(plans, "y", room=0) is None
    assert list(plans) == list(range(50))


def test_a_miss_below_room_leaves_the_dict_unchanged():
    plans = {"a": 1, "b": 2, "c": 3}
    assert cached(plans, "x", room=4) is None
    assert list(plans.items()) == [("a", 1), ("b", 2), ("c", 3)]
    assert cached({}, "x", room=1) is None


# ------------------------------------------------------------------------------------------ the identity of a training forward
@pytest.fixture
def eng():
    return UNetModel(args=make_args(), **SMALL).train().train_engine


def _refused(eng, forward, detail=None):
    """``backward(forward=...)`` raises the RuntimeError - before it reads ``dout`` (None here), a plan buffer or a ``param.grad``."""
    with pytest.raises(RuntimeError, match="a later forward on this model overwrote the activations this backward needs") as e:
        eng.backward(None, forward=forward)
    text = str(e.value)
    assert "one forward per" in text.lower() and "torch.no_grad()" in text and "model.eval()" in text
    assert (detail in text) if detail else ("released" not in text)


def test_the_identity_matches_until_the_next_forward(eng):
    P = TrainPlan()
    eng._tplans["k"] = P
    assert eng.last_forward() is None and eng.holds_plan(P) and not eng.holds_plan(None) and not eng.holds_plan(TrainPlan())
    ident = eng.claim_forward(P)
    assert ident == (P, 1) and eng.last_forward() == ident and eng._live is P and P.serial == 1
    assert eng._check_forward(ident) is P
    assert eng._check_forward(ident) is P  # checking consumes nothing: a second backward through one forward is allowed


def test_a_later_forward_on_the_same_plan_makes_the_identity_stale(eng):
    P = TrainPlan()
    eng._tplans["k"] = P
    first = eng.claim_forward(P)
    second = eng.claim_forward(P)  # same shape: the same cached plan, its intermediates overwritten
    assert first[0] is second[0] and first[1] != second[1]
    _refused(eng, first)
    assert eng._check_forward(second) is P  # the later forward is still differentiable, also after the refusal


def test_a_dropped_plan_is_refused_whatever_is_live(eng):
    P, Q = TrainPlan(), TrainPlan()
    eng._tplans["k"] = P
    first = eng.claim_forward(P)
    eng._tplans.clear()  # what plan_train does when another key is asked for
    eng._tplans["k2"] = Q
    _refused(eng, first, "released")  # (P is still ``_live``: no forward has run on Q yet)
    second = eng.claim_forward(Q)
    _refused(eng, first, "released")
    assert eng._check_forward(second) is Q
    # the plan of the old key built again is another object: the old identity stays stale
    eng._tplans.clear()
    eng._tplans["k"] = P2 = TrainPlan()
    eng.claim_forward(P2)
    _refused(eng, first, "released")
    _refused(eng, second, "released")


def test_backward_without_an_identity_needs_a_live_held_plan(eng):
    with pytest.raises(RuntimeError, match="backward without a training forward"):
        eng.backward(torch.zeros(1), assign=False)
    P = TrainPlan()
    eng._tplans["k"] = P
    eng.claim_forward(P)
    eng._tplans.clear()
    with pytest.raises(RuntimeError, match="released"):
        eng.backward(torch.zeros(1), assign=False)
