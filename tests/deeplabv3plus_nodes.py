"""
DeepLabV3Plus's part of the node-level oracle (tests/deeplabv3_nodes.py holds the Recorder, the shared node kinds and every float64
reference): the schedule of DeepLabV3PlusMI355X._forward_native, the names py4cast_amd/deeplabv3plus.py binds, and two more node kinds --

  "dw"    deeplabv3plus.depthwise3x3_dilated: x -> y_0 .. y_{R-1}; ONE node owns the R depthwise weights ``w0`` .. ``w{R-1}`` (R = 3 for
          the ASPP's three rates -- its scheduled module is a ModuleList of the three depthwise convolutions --, 1 for decoder.aspp.1.0
          and decoder.block2.0.0);
  "upcat" deeplabv3plus.up_cat: a, skip -> out (ld = dc + 48); no parameters.

deeplabv3plus.py imports stem_tail, aspp_assemble and upsample_bilinear_ac BY NAME, so the patches go on that module's own names (a patch
of py4cast_amd.deeplabv3.<name> would not reach them), and ``_patch`` is a staticmethod bound when the class was created: patched on
DeepLabV3PlusMI355X itself.
"""
from torch import nn

import deeplabv3_nodes as N
from unet_nodes import param_of

KINDS = N.KINDS + ("dw", "upcat")
GRAD_SLOTS = {**N.GRAD_SLOTS, "dw": {"x": 0, "w0": 2, "w1": 3, "w2": 4}, "upcat": {"a": 0, "skip": 1}}
DIFF_INPUTS = {**N.DIFF_INPUTS, "dw": ("x",), "upcat": ("a", "skip")}
PLACED = ("up", "upcat")        # kinds whose call names no module: their place in the schedule identifies them


def schedule(model):
    """[(kind, name, module)] in the order DeepLabV3PlusMI355X._forward_native calls its nodes (the bf16 route).  A "dw" entry's module
    is a ModuleList of its R depthwise convolutions (built here: it is not a submodule of the model)."""
    s = N.encoder_schedule(model)
    s.insert(1, ("stem", "encoder.bn1"))
    s = [(k, n, model.get_submodule(n)) for k, n in s]
    a = "decoder.aspp.0"
    aspp = model.decoder.aspp[0]

    def sub(kind, name):
        return (kind, name, model.get_submodule(name))

    s += [sub("conv", f"{a}.convs.0.0"), sub("bn", f"{a}.convs.0.1"),
          ("dw", f"{a}.convs.1-3.0.0", nn.ModuleList([aspp.convs[k][0][0] for k in (1, 2, 3)]))]
    for k in (1, 2, 3):
        s += [sub("conv", f"{a}.convs.{k}.0.1"), sub("bn", f"{a}.convs.{k}.1")]
    s += [sub("aspp", f"{a}.convs.4"), sub("conv", f"{a}.project.0"), sub("bn", f"{a}.project.1"),
          ("dw", "decoder.aspp.1.0", nn.ModuleList([model.decoder.aspp[1][0]])), sub("conv", "decoder.aspp.1.1"), sub("bn", "decoder.aspp.2"),
          sub("conv", "decoder.block1.0"), sub("bn", "decoder.block1.1"), ("upcat", "decoder.up", None),
          ("dw", "decoder.block2.0.0", nn.ModuleList([model.decoder.block2[0][0]])), sub("conv", "decoder.block2.0.1"), sub("bn", "decoder.block2.1"),
          sub("conv", "segmentation_head.0"), ("up", "segmentation_head.1", None)]
    return s


class Description(N.Description):
    label = "DeepLabV3PlusMI355X"
    kinds, grad_slots, diff_inputs = KINDS, GRAD_SLOTS, DIFF_INPUTS

    def schedule(self, model):
        return schedule(model)

    def params(self, node):
        if node.kind == "dw":
            return {f"w{r}": conv.weight for r, conv in enumerate(node.module)}
        if node.kind in PLACED:
            return {}
        return super().params(node)

    def check_owner(self, kind, name, owner, module):
        if kind == "dw":
            assert len(owner) == len(module), f"{name}: {len(owner)} rates in the call, {len(module)} scheduled"
            for r, (w, conv) in enumerate(zip(owner, module)):
                assert param_of(w) is conv.weight, f"{name}: the call's weight {r} is not the scheduled depthwise convolution's"
        elif kind not in PLACED:
            super().check_owner(kind, name, owner, module)

    def install(self, rec):
        from py4cast_amd import deeplabv3 as D
        from py4cast_amd import deeplabv3plus as DP

        cls = DP.DeepLabV3PlusMI355X
        assert "_patch" in cls.__dict__, "DeepLabV3PlusMI355X binds its own _patch"
        rec.patch(cls, "_patch", staticmethod(rec.wrap_patch(cls._patch)))
        rec.patch(DP, "stem_tail", rec.wrap_stem(DP.stem_tail))
        rec.patch(DP, "aspp_assemble", rec.wrap_aspp(DP.aspp_assemble))
        rec.patch(DP, "upsample_bilinear_ac", rec.wrap_up(DP.upsample_bilinear_ac))
        dw0, upcat0 = DP.depthwise3x3_dilated, DP.up_cat

        def depthwise3x3_dilated(x, weights, rates):
            ws = list(weights)
            node = rec._begin("dw", ws, {"x": x, **{f"w{r}": w for r, w in enumerate(ws)}}, {"rates": tuple(int(d) for d in rates)})
            ys = dw0(x, ws, rates)
            rec._end(node, list(ys), ys[0].grad_fn)
            return ys

        def up_cat(a, skip, scale, ld=None):
            node = rec._begin("upcat", None, {"a": a, "skip": skip}, {"scale": int(scale), "ld": ld})
            out = upcat0(a, skip, scale, ld)
            node.opts["ld"] = out.shape[-1]
            rec._end(node, [out], out.grad_fn)
            return out

        rec.patch(DP, "depthwise3x3_dilated", depthwise3x3_dilated)
        rec.patch(DP, "up_cat", up_cat)
        for fn_cls in (D._StemTail, D._AsppAssemble, D._UpsampleAC, DP._DepthwiseDilated, DP._UpCat):
            rec.wrap_backward(fn_cls)


def counts(model):
    return Description().counts(model)


def Recorder(model):
    return N.Recorder(model, Description())


def owned_parameters(model):
    """the ids of the parameters of every scheduled module (tests: each of the model's parameters exactly once)"""
    return [id(p) for _, _, mod in schedule(model) if mod is not None for p in mod.parameters()]

