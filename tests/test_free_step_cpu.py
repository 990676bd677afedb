"""CPU checks of the loss-free AR step's plumbing: the new entry points are declared in include/py4cast_hip.h, typed in
py4cast_amd/_lib.py with the header's arity, exported by the library and counted as native time by the HalfUNet; and the
constructor still refuses the combinations the K >= 2 schedule is not defined for."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("p4c_ar_update_next", "p4c_out_conv_update_fwd", "p4c_ar_update_next_bwd")


def _header_arity(name):
    src = open(os.path.join(ROOT, "include", "py4cast_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in include/py4cast_hip.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", NEW)
def test_free_step_entry_points_are_declared_typed_exported_and_timed(name):
    from py4cast_amd import _lib
    from py4cast_amd.halfunet import HalfUNetMI355X

    assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[name]) == _header_arity(name)
    assert hasattr(_lib.lib(), name)
    assert name in HalfUNetMI355X(21, 12, (32, 32)).timed_entry_points


def test_inter_steps_constructor_refusals_are_unchanged():
    from helpers import make_dataset_info, synthetic_case
    from py4cast_amd.lightning import AutoRegressiveLightning

    case = synthetic_case(seed=1, B=1, T=1, T_in=1, H=16, W=16, F=4, Ff=5, Fs=4)
    info = make_dataset_info(case, 5)
    kw = dict(batch_size=1, model_name="HalfUNet", num_pred_steps_train=1,
              losses=[{"class": "WeightedLoss", "params": {"loss": "MSELoss", "reduction": "none"}}])
    with pytest.raises(AttributeError):
        AutoRegressiveLightning({}, info, None, num_input_steps=2, num_inter_steps=2, training_strategy="scaled_ar", **kw)
    lm = AutoRegressiveLightning({}, info, None, num_input_steps=1, num_inter_steps=2, training_strategy="diff_ar", **kw)
    with pytest.raises(ValueError):   # diff_ar raises for K != 1 where the reference does: when the strategy is resolved
        lm._strategy_params()
    lm = AutoRegressiveLightning({}, info, None, num_input_steps=1, num_inter_steps=2, training_strategy="scaled_ar", **kw)
    assert lm._strategy_params() == (True, True, 2)
