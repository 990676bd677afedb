"""
CustomUNet (py4cast_amd/customunet.py) node by node: one forward / backward of CustomUNetMI355X's bf16 route under the recorder of
tests/deeplabv3_nodes.py with tests/customunet_nodes.py's description, then for every recorded node (7 strided patch convolutions, 24
implicit-GEMM convolutions with their passthrough / bias, 29 batch norms with their residual, the stem tail with its skip output, the
four nearest-x2 + concatenation passes and the in-place one of decoder block 3 -- resnet18; resnet34: 40 and 45) the checks of
tests/test_deeplabv3_nodes_gpu.py (tests/encoder_nodes_checks.py holds them, with the bars):

* replay: the node alone on its recorded inputs and incoming gradients, with fresh parameter leaves, gives the in-network outputs and
  input / parameter gradients BIT FOR BIT, the stem's routing table and the running statistics included.  The stem's buffer output is
  compared from its channel offset on (its first 64 channels are uninitialised until up2_into fills them); up2into's replay starts
  from a copy of the recorded buffer;
* float64: the replay against the float64 node reference, forward on the reference's own decisions, gradients with every decision
  (ReLU masks, the stem's routing table) from the device; an eval-mode forward of every batch norm, the stem's two outputs included;
* wiring: every node input but the network's own is a recorded output; single-consumer edges bit-identical; f2, f3 and f4 each have
  THREE consumers (the next layer's conv1, its downsample, a decoder skip) whose gradients sum; the in-place edge: up2into's buf is
  the stem's output 0 and decoder.blocks.3.conv1.0 reads up2into's output; the stem's incoming buffer gradient is what up2into handed
  on, which is decoder.blocks.3.conv1.0's dx -- and the stem reads only its own channels of it: replayed with the first 64 channels of
  that gradient replaced by NaN, its gradients do not change by a bit;
* every parameter belongs to exactly one node and the network's p.grad is that node replay's gradient;
* sink route: the same backward with every .grad pre-filled, and under FlatDDP with a non-zero flat buffer: p.grad = prefill + the
  gradient of the first run, bit for bit.

Cases: three toys (resnet18, resnet34 at 64 x 96, B = 3) and the Titan grid (2 x 512 x 640, 46 -> 21): decoder block 4's up2_cat
covers 2 * 256 * 320 * 4 = 655360 octets, more than the 524288 one trip of the grid-stride loop covers -- the smallest real grid whose
in-network launch takes a second trip.

Measured at the Titan grid (resnet18: 66 nodes; worst node / bar): bf16 maps 5.3e-3 / 6e-3 per element and 2.3e-3 / 3e-3 in the 2-norm
(bf16 rounding of the stored maps), convolution weight / bias gradients 2.6e-6 / 5e-4, BN gamma / beta gradients 2.3e-7 / 5e-3, stem tail
4.9e-7 / 3e-3, running mean / var 5.7e-8 / 1e-4, statistics epilogues 5.2e-8 / 1e-5, up2cat / up2into dx 1.0 of its bound (a sum that
lands half-way between two bf16 values is exactly half an ulp off: the bound is attained, not exceeded).  The toys measure the same to
within a factor of two.  The whole file takes about 10 s on one MI355X.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import customunet_nodes as M  # noqa: E402
import encoder_nodes_checks as K  # noqa: E402

pytestmark = pytest.mark.gpu

# name -> (B, H, W, in_channels, out_channels, encoder)
CASES = {
    "toy-r18": (2, 64, 64, 69, 60, "resnet18"),
    "toy-r34-64x96": (2, 64, 96, 69, 60, "resnet34"),
    "toy-r18-b3": (3, 64, 64, 69, 60, "resnet18"),
    "titan": (2, 512, 640, 46, 21, "resnet18"),     # the Titan grid; 46 input channels -> 48
}
SEED = 5
GRID_CAP_OCTETS = 2048 * 256      # csrc/customunet.hip: at most 2048 workgroups of 256 threads, one octet per thread and trip
COUNTS = {"resnet18": {"patch": 7, "conv": 24, "bn": 29, "stemskip": 1, "up2cat": 4, "up2into": 1},
          "resnet34": {"patch": 7, "conv": 40, "bn": 45, "stemskip": 1, "up2cat": 4, "up2into": 1}}


def make_model(case, dev):
    from py4cast_amd.customunet import CustomUNetMI355X, CustomUNetSettings

    B, H, W, cin, cout, enc = CASES[case]
    torch.manual_seed(0)
    m = CustomUNetMI355X(cin, cout, (H, W), CustomUNetSettings(encoder_name=enc, encoder_weights=False, compute_dtype="bf16",
                                                               activation_dtype="bf16")).to(dev).train()
    K.randomise(m)
    return (m,) + K.inputs(B, H, W, cin, cout, dev)


@pytest.fixture(scope="module", params=list(CASES))
def run(request, gpu_device):
    torch.cuda.empty_cache()
    m, x, dy = make_model(request.param, gpu_device)
    ns = K.record(request.param, m, x, dy, M.Recorder, SEED)
    yield ns
    del m, ns
    torch.cuda.empty_cache()


def test_replay_is_bit_identical(run):
    got = {k: sum(n.kind == k for n in run.rec.nodes) for k in M.KINDS}
    assert got == COUNTS[CASES[run.case][5]], got
    K.check_replay_is_bit_identical(run)


def test_nodes_against_float64(run):
    if run.case == "titan":
        # decoder block 4's up2_cat (no skip): past one trip of the grid-stride loop, forward and backward
        n = run.rec["decoder.blocks.4.up"]
        B, h, w, Cx = n.args["x"].shape
        assert (B, h, w, Cx) == (2, 256, 320, 32) and n.args["skip"] is None and B * h * w * (Cx // 8) == 655360 > GRID_CAP_OCTETS
    K.check_nodes_against_float64(run)


def test_wiring(run):
    rec, m = run.rec, run.model
    multi = K.check_edges(run, M.DIFF_INPUTS)
    last = K.last_blocks(m)
    want = {last[1]: sorted(["encoder.layer2.0.conv1 x", "encoder.layer2.0.downsample.0 x", "decoder.blocks.2.up skip"]),
            last[2]: sorted(["encoder.layer3.0.conv1 x", "encoder.layer3.0.downsample.0 x", "decoder.blocks.1.up skip"]),
            last[3]: sorted(["encoder.layer4.0.conv1 x", "encoder.layer4.0.downsample.0 x", "decoder.blocks.0.up skip"])}
    assert multi == want, multi
    # the in-place edge
    names = [n.name for n in rec.nodes]
    stem, into, conv = rec["encoder.bn1"], rec["decoder.blocks.3.up"], rec["decoder.blocks.3.conv1.0"]
    i_stem, i_into = names.index("encoder.bn1"), names.index("decoder.blocks.3.up")
    assert stem.kind == "stemskip" and into.kind == "up2into"
    assert into.src["buf"] == (i_stem, 0) and conv.src["x"] == (i_into, 0)
    assert rec["encoder.layer1.0.conv1"].src["x"] == (i_stem, 1) and into.src["x"] == (names.index("decoder.blocks.2.conv2.1"), 0)
    off = stem.opts["offset"]
    assert off == into.args["x"].shape[-1] == 64 and stem.out[0].shape[-1] == 128
    K.same(into.gout[0], conv.grad("x"), "decoder.blocks.3.conv1.0 dx -> up2into")
    K.same(stem.gout[0], into.grad("buf"), "up2into's handed-on gradient -> the stem")
    K.same(stem.gout[0], conv.grad("x"), "the stem receives the whole 128-wide gradient of the buffer")
    assert bool(stem.gout[0][..., :off].any()), "the first channels of the buffer's gradient are the up-sampling's, not zeros"
    # ... of which the stem reads only its own slice: the same replay with the other channels poisoned
    poisoned = stem.gout[0].clone()
    poisoned[..., :off] = float("nan")
    _, g0, _, _ = K.replays(run)[i_stem]
    _, g1, _, _ = K.replay(stem, gout=[poisoned, stem.gout[1]])
    for slot in ("y", "gamma", "beta"):
        K.same(g1[slot], g0[slot], f"the stem's d{slot} with the first {off} channels of its buffer gradient poisoned")
    K.check_head_gradient(run, rec["segmentation_head.0"])


def test_parameter_gradients_are_the_node_replays(run):
    K.check_parameter_gradients_are_the_node_replays(run)


def test_sink_route_adds_into_grad(run):
    K.check_sink_route_adds_into_grad(run)
