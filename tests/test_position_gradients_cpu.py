"""CPU-side checks (no GPU) of the `position_gradients` switch of the system models: a plain class attribute that is off by default,
travels in a pickle only when it was set, and reads False on a model restored from a state that predates it."""
import pickle

import pytest

PARAMS = {'size': 3, 'aggregation': 'sum', 'message_passing_steps': 1,
          'rmp': {'clustering': 'none', 'connector': 'none', 'num_clusters': 3, 'hyper_noise': 'none', 'hyper_node_features': True,
                  'frequency': 1, 'fully_connect': False, 'intra_cluster_sampling': {'enabled': False, 'alpha': 0.1, 'spotter_threshold': 0}},
          'graph_balancer': {'algorithm': 'none', 'frequency': 1}}


def _classes():
    from hgn_amd import system_model
    return system_model.FlagModel, system_model.CylinderModel, system_model.PlateModel


def test_position_gradients_is_off_by_default_on_the_three_models():
    from hgn_amd import system_model
    assert system_model.AbstractSystemModel.position_gradients is False
    for cls in _classes():
        assert cls.position_gradients is False and 'position_gradients' not in vars(cls)        # inherited, not redefined
        assert cls(PARAMS).position_gradients is False
    assert system_model.PlateModel._LOCKSTEP.differentiable is False                             # the record stays as it was


@pytest.mark.parametrize('index', [0, 1, 2], ids=['flag', 'cylinder', 'plate'])
def test_a_model_from_a_state_without_the_attribute_reads_false(index):
    cls = _classes()[index]
    model = cls(PARAMS)
    state = model.__getstate__()
    assert 'position_gradients' not in state                   # a class attribute: the states of old pickles look like this one
    old = cls.__new__(cls)
    old.__setstate__(state)
    assert old.position_gradients is False
    assert pickle.loads(pickle.dumps(model)).position_gradients is False
    model.position_gradients = True                            # once set it is instance state and travels
    assert 'position_gradients' in model.__getstate__()
    assert pickle.loads(pickle.dumps(model)).position_gradients is True
    assert cls(PARAMS).position_gradients is False             # and it was set on that one model only
