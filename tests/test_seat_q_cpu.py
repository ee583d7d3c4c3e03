"""CPU: the role map of the per-role Q forward (dqn_glue.role_slots, RoleQ, SeatLoop, compete) -- slot sharing and the argument
errors, all raised before any device call."""
import importlib

import pytest
import torch


@pytest.fixture(scope="module")
def glue():
    return importlib.import_module("doudizhu-rl_amd.dqn_glue")


def _net(glue, P, seed=0):
    torch.manual_seed(seed)
    return glue.QNet(P).eval()


def test_equal_networks_share_a_slot(glue):
    A, B = _net(glue, 9, 1), _net(glue, 9, 2)
    assert glue.role_slots({"down": B, "up": B}, 2) == ([B], [0, -1, 0])
    slots, m = glue.role_slots({"lord": A, "down": B, "up": A}, 2)
    assert slots == [A, B] and m == [0, 0, 1]
    slots, m = glue.role_slots({"lord": A}, 2)
    assert slots == [A] and m == [-1, 0, -1]
    # a copy with equal weights is another network: its own slot
    C = _net(glue, 9, 1)
    assert len(glue.role_slots({"lord": A, "up": C}, 2)[0]) == 2


def test_argument_errors(glue):
    A, B6 = _net(glue, 9), _net(glue, 6)
    A7 = _net(glue, 7)
    with pytest.raises(ValueError, match="differ"):
        glue.role_slots({"lord": A, "down": B6}, 2)
    with pytest.raises(ValueError, match="planes"):
        glue.role_slots({"lord": A}, 3)
    with pytest.raises(ValueError, match="planes"):
        glue.role_slots({"lord": A7}, 2)
    for v in (0, 4):
        with pytest.raises(ValueError, match="variant"):
            glue.role_slots({"lord": A}, v)
    with pytest.raises(ValueError, match="unknown role"):
        glue.role_slots({"landlord": A}, 2)
    with pytest.raises(ValueError, match="no network"):
        glue.role_slots({"lord": None, "down": None}, 2)
    with pytest.raises(ValueError, match="no network"):
        glue.role_slots({}, 2)
    # the same checks guard RoleQ and SeatLoop before anything touches a device
    with pytest.raises(ValueError, match="variant"):
        glue.RoleQ({"lord": A}, 0)
    with pytest.raises(ValueError, match="unknown role"):
        glue.SeatLoop(None, {"farmer": A}, 2)
