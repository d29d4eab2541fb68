"""engine._mlp_args: the one marshaller of set_policy_mlp, actor_set and critic_set checks every layer's shape before the library sees a
pointer.  No batch and no device."""
import re

import numpy as np
import pytest

from humanoid_mujoco_amd.engine import _mlp_args

SIZES = [48, 33, 17, 21]
TEXT = "weights[l] must be [sizes[l], sizes[l+1]] and biases[l] [sizes[l+1]]"


def _net(sizes=SIZES):
    rng = np.random.default_rng(3)
    return ([rng.uniform(-1, 1, size=(a, c)) for a, c in zip(sizes[:-1], sizes[1:])], [rng.uniform(-1, 1, size=c) for c in sizes[1:]])


@pytest.mark.parametrize("sizes", [None, SIZES])
def test_consistent_set_is_marshalled(sizes):
    weights, biases = _net()
    ws, bs, csz, wp, bp = _mlp_args("set_policy_mlp", weights, biases, sizes)
    assert list(csz) == SIZES and len(wp) == len(bp) == 3
    for l in range(3):
        assert ws[l].dtype == np.float32 and ws[l].flags.c_contiguous and np.array_equal(ws[l], weights[l].astype(np.float32))
        assert bs[l].dtype == np.float32 and np.array_equal(bs[l], biases[l].astype(np.float32))
        assert wp[l] == ws[l].ctypes.data and bp[l] == bs[l].ctypes.data


@pytest.mark.parametrize("sizes", [None, SIZES])
def test_bias_of_the_wrong_length(sizes):
    weights, biases = _net()
    biases[1] = np.zeros(18)
    with pytest.raises(ValueError, match=re.escape("critic_set: " + TEXT)):
        _mlp_args("critic_set", weights, biases, sizes)


def test_rows_that_do_not_match_the_previous_columns():
    """sizes derived from the shapes (set_policy_mlp): weights[1] with 34 rows behind 33 columns would be read past its end."""
    weights, biases = _net()
    weights[1] = np.zeros((34, 17))
    with pytest.raises(ValueError, match="set_policy_mlp: "):
        _mlp_args("set_policy_mlp", weights, biases)
    with pytest.raises(ValueError, match="actor_set: "):
        _mlp_args("actor_set", weights, biases, SIZES)


@pytest.mark.parametrize("sizes", [None, SIZES])
def test_fewer_biases_than_weights(sizes):
    weights, biases = _net()
    with pytest.raises(ValueError):
        _mlp_args("actor_set", weights, biases[:2], sizes)
    with pytest.raises(ValueError):
        _mlp_args("actor_set", weights, biases + [np.zeros(21)], sizes)
