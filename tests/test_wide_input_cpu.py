"""
HalfUNet inputs of num_input_steps >= 2 past states (in_channels = T_in * F + Fs + Ff): construction limits of the fused plan
(cin_pad up to 256) and the number of leading input channels whose gradient the plan returns.  No GPU needed.
"""
import pytest


@pytest.mark.parametrize("cin,cout", [(129, 60), (189, 60), (256, 64)])
def test_wide_inputs_construct(cin, cout):
    from py4cast_amd.halfunet import HalfUNetMI355X

    m = HalfUNetMI355X(cin, cout, (64, 64))
    assert not m.module_path
    assert m.cin_pad == (cin + 31) // 32 * 32
    assert m.grad_input_channels == cin   # beyond 96 inputs: the gradient of every input channel by default
    assert m.dx_width == 64 * ((cin + 63) // 64)
    assert m.encoder1.enc1conv1.weight.shape == (64, cin, 3, 3)


@pytest.mark.parametrize("cin,cout,limit", [(257, 60, "in_channels=257 > 256"), (100, 65, "out_channels=65 > 64")])
def test_wide_inputs_beyond_the_limits_raise(cin, cout, limit):
    from py4cast_amd.halfunet import HalfUNetMI355X

    with pytest.raises(NotImplementedError, match=limit):
        HalfUNetMI355X(cin, cout, (64, 64))


def test_narrow_inputs_keep_their_gradient_width():
    from py4cast_amd.halfunet import HalfUNetMI355X

    assert HalfUNetMI355X(69, 60, (64, 64)).grad_input_channels == 64
    assert HalfUNetMI355X(46, 21, (64, 64)).grad_input_channels == 46
    assert HalfUNetMI355X(89, 40, (64, 64)).grad_input_channels == 64
    m = HalfUNetMI355X(89, 40, (64, 64))
    m.grad_input_channels = 80
    assert m.grad_input_channels == 80 and m.dx_width == 128
    with pytest.raises(ValueError):
        m.grad_input_channels = 90


def _lightning(F, T_in, strategy="scaled_ar"):
    from helpers import make_dataset_info, synthetic_case
    from py4cast_amd.lightning import AutoRegressiveLightning

    case = synthetic_case(seed=1, B=2, T=2, T_in=T_in, H=32, W=32, F=F, Ff=5, Fs=4)
    info = make_dataset_info(case, 5)
    return AutoRegressiveLightning(
        {}, info, None, num_input_steps=T_in, num_pred_steps_train=2, batch_size=2, model_name="HalfUNet",
        losses=[{"class": "WeightedLoss", "weight": 1.0, "params": {"loss": "MSELoss", "reduction": "none"}}],
        training_strategy=strategy,
    )


@pytest.mark.parametrize("F,T_in,in_channels,expected", [(40, 2, 89, 80), (60, 1, 69, 64), (60, 2, 129, 129), (12, 3, 45, 45)])
def test_lightning_sets_the_gradient_width_to_every_past_state(F, T_in, in_channels, expected):
    lm = _lightning(F, T_in)
    assert lm.model.in_channels == in_channels
    assert lm.model.grad_input_channels == expected
    assert lm.model.grad_input_channels >= T_in * F
