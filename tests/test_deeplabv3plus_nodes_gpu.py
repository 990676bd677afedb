"""
DeepLabV3Plus (py4cast_amd/deeplabv3plus.py) node by node: one forward / backward of DeepLabV3PlusMI355X's bf16 route under the
recorder of tests/deeplabv3_nodes.py with tests/deeplabv3plus_nodes.py's description, then for every recorded node (5 strided patch
convolutions, 24 implicit-GEMM convolutions with their dilation / passthrough / bias, 27 batch norms with their residual and Dropout
multiplier, the stem tail, 3 depthwise nodes -- the ASPP's three rates are ONE node that owns three weights --, the ASPP assembly, the
bilinear x4 + concatenation pass and the head's x4 up-sampling -- resnet18; resnet34: 40 and 43) the checks of
tests/test_deeplabv3_nodes_gpu.py (tests/encoder_nodes_checks.py holds them, with the bars):

* replay: the node alone on its recorded inputs and incoming gradients, with fresh parameter leaves, gives the in-network outputs and
  input / parameter gradients BIT FOR BIT, the stem's routing table and the running statistics included; the three-rate depthwise
  node is replayed as one three-rate call;
* float64: the replay against the float64 node reference, forward on the reference's own decisions, gradients with every decision
  (ReLU masks, the stem's routing table, the Dropout draw = model.last_dropout_mask with mul_factor = 1 / (1 - p)) from the device;
  the depthwise weights as given (the kernel reads the fp32 masters); an eval-mode forward of every batch norm;
* wiring: every node input but the network's own is a recorded output; single-consumer edges bit-identical; layer1's output has
  THREE consumers (layer2.0's conv1 and downsample, decoder.block1.0), layer4's too (the ASPP's 1x1 branch, the three-rate depthwise
  launch, the pooling branch), layer2's and layer3's two: their gradients equal the float64 sum within the bf16 roundings of the adds;
* every parameter belongs to exactly one node slot and the network's p.grad is that node replay's gradient;
* sink route: the same backward with every .grad pre-filled, and under FlatDDP with a non-zero flat buffer: p.grad = prefill + the
  gradient of the first run, bit for bit, with the same Dropout draw.

The ASPP pooling branch's batch norm at B = 2 is eps-driven: the scaled bounds tests/test_deeplabv3_nodes_gpu.py derives for it, with
H W of the stride-16 map; the B = 3 case holds it to the ordinary bars.

Cases: four toys (dc = 64; p = 0 and 0.5, resnet34 at 64 x 96, B = 3) and ``trips`` (2 x 512 x 256, dc = 256, p = 0.5): the stride-4 map
has 2 * 128 * 64 = 16384 pixels x 38 octets = 622592 > 524288, so block2's depthwise forward and data gradient and up_cat take a second
trip of their grid-stride loops in the network; 16384 pixels also put dw_wgrad on its 128-pixel blocks while the stride-16 launches
(1024 pixels) stay on the 64-pixel ones.

Measured at ``trips`` (resnet18: 63 nodes; worst node / bar): bf16 maps 4.6e-3 / 6e-3 per element and 2.3e-3 / 3e-3 in the 2-norm (bf16
rounding of the stored maps), convolution weight / bias gradients 5.4e-7 / 5e-4, dilated 3x3 weight gradients 2.1e-7 / 3e-3, depthwise
weight gradients 2.2e-7 / 5e-4, BN gamma / beta gradients 3.7e-6 / 5e-3, stem tail 3.7e-7 / 3e-3, running mean / var 3.0e-7 / 1e-4,
statistics epilogues 5.0e-8 / 1e-5; the ASPP pooling branch at B = 2: dx 2.4e-4 / 6e-3 and dw 6.8e-6 / 5e-4 of their scales (the B = 3
toy: within the ordinary bars, its 1x1 weight gradient 1.0e-5 / 5e-4).  The whole file takes about 6 s on one MI355X.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import deeplabv3plus_nodes as M  # noqa: E402
import encoder_nodes_checks as K  # noqa: E402

pytestmark = pytest.mark.gpu

# name -> (B, H, W, in_channels, out_channels, encoder, decoder_channels, aspp_dropout)
CASES = {
    "toy-r18-p0": (2, 64, 64, 69, 60, "resnet18", 64, 0.0),
    "toy-r18-p05": (2, 64, 64, 69, 60, "resnet18", 64, 0.5),
    "toy-r34-64x96": (2, 64, 96, 69, 60, "resnet34", 64, 0.0),
    "toy-r18-b3": (3, 64, 64, 69, 60, "resnet18", 64, 0.0),
    "trips": (2, 512, 256, 69, 60, "resnet18", 256, 0.5),
}
SEED = 5        # the generator state every forward starts from (the Dropout draw)
GRID_CAP_OCTETS = 2048 * 256      # csrc/deeplabplus.hip: at most 2048 workgroups of 256 threads, one octet per thread and trip
COUNTS = {"resnet18": {"patch": 5, "conv": 24, "bn": 27, "stem": 1, "aspp": 1, "up": 1, "dw": 3, "upcat": 1},
          "resnet34": {"patch": 5, "conv": 40, "bn": 43, "stem": 1, "aspp": 1, "up": 1, "dw": 3, "upcat": 1}}


def make_model(case, dev):
    from py4cast_amd.deeplabv3plus import DeepLabV3PlusMI355X, DeepLabV3PlusSettings

    B, H, W, cin, cout, enc, dc, p = CASES[case]
    torch.manual_seed(0)
    m = DeepLabV3PlusMI355X(cin, cout, (H, W), DeepLabV3PlusSettings(encoder_name=enc, decoder_channels=dc, encoder_weights=False, aspp_dropout=p,
                                                                     compute_dtype="bf16", activation_dtype="bf16")).to(dev).train()
    K.randomise(m)
    return (m,) + K.inputs(B, H, W, cin, cout, dev)


@pytest.fixture(scope="module", params=list(CASES))
def run(request, gpu_device):
    torch.cuda.empty_cache()
    m, x, dy = make_model(request.param, gpu_device)
    ns = K.record(request.param, m, x, dy, M.Recorder, SEED, dropout_p=CASES[request.param][7])
    assert (ns.mask is not None) == (ns.dropout_p > 0)
    yield ns
    del m, ns
    torch.cuda.empty_cache()


def test_replay_is_bit_identical(run):
    got = {k: sum(n.kind == k for n in run.rec.nodes) for k in M.KINDS}
    assert got == COUNTS[CASES[run.case][5]], got
    assert [len(n.opts["rates"]) for n in run.rec.nodes if n.kind == "dw"] == [3, 1, 1]
    assert run.rec.nodes[[n.kind for n in run.rec.nodes].index("dw")].opts["rates"] == (12, 24, 36)
    K.check_replay_is_bit_identical(run)


def test_nodes_against_float64(run):
    from py4cast_amd import _lib as L

    if run.case == "trips":
        # the stride-4 map: block2's depthwise launches and up_cat past one trip; dw_wgrad on 128-pixel blocks there, on 64-pixel ones
        # at stride 16
        n, u, a3 = run.rec["decoder.block2.0.0"], run.rec["decoder.up"], run.rec["decoder.aspp.0.convs.1-3.0.0"]
        B, H, W, C = n.args["x"].shape
        assert (B, H, W, C) == (2, 128, 64, 304) and B * H * W == 16384 and B * H * W * (C // 8) == 622592 > GRID_CAP_OCTETS
        assert u.out[0].shape == (2, 128, 64, 304) and u.opts["ld"] == 304
        assert L.lib().p4c_dlp_dw3x3_wgrad_rows(B, H, W) == 16384 // 128
        b, h, w, c = a3.args["x"].shape
        assert (b, h, w, c) == (2, 32, 16, 512) and L.lib().p4c_dlp_dw3x3_wgrad_rows(b, h, w) == 1024 // 64
    K.check_nodes_against_float64(run)


def test_wiring(run):
    rec, m = run.rec, run.model
    multi = K.check_edges(run, M.DIFF_INPUTS)
    last = K.last_blocks(m)
    want = {last[1]: sorted(["encoder.layer2.0.conv1 x", "encoder.layer2.0.downsample.0 x", "decoder.block1.0 x"]),
            last[2]: ["encoder.layer3.0.conv1 x", "encoder.layer3.0.downsample.0 x"],
            last[3]: ["encoder.layer4.0.conv1 x", "encoder.layer4.0.downsample.0 x"],
            last[4]: sorted(["decoder.aspp.0.convs.0.0 x", "decoder.aspp.0.convs.1-3.0.0 x", "decoder.aspp.0.convs.4 x"])}
    assert multi == want, multi
    # the three rates' maps each go to their own pointwise convolution; up_cat's inputs are aspp.2's and block1.1's outputs
    names = [n.name for n in rec.nodes]
    i_dw = names.index("decoder.aspp.0.convs.1-3.0.0")
    for k in (1, 2, 3):
        assert rec[f"decoder.aspp.0.convs.{k}.0.1"].src["x"] == (i_dw, k - 1)
    up = rec["decoder.up"]
    assert up.src["a"] == (names.index("decoder.aspp.2"), 0) and up.src["skip"] == (names.index("decoder.block1.1"), 0)
    K.check_head_gradient(run, rec["segmentation_head.1"])


def test_parameter_gradients_are_the_node_replays(run):
    K.check_parameter_gradients_are_the_node_replays(run)


def test_sink_route_adds_into_grad(run):
    K.check_sink_route_adds_into_grad(run)
