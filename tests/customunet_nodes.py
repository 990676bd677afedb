"""
CustomUNet's part of the node-level oracle (tests/deeplabv3_nodes.py holds the Recorder, the shared node kinds and every float64
reference): the schedule of CustomUNetMI355X._forward_native, the names py4cast_amd/customunet.py binds, and three more node kinds --

  "stemskip" customunet.stem_tail_skip: y, stats -> buf, pool; saved: the ``arg`` routing table; owns bn1's gamma and beta.  buf
             (B, H, W, offset + 64) holds f1 from channel ``offset`` on; its first ``offset`` channels are UNINITIALISED when the recorder
             clones it: every comparison of that output covers [..., offset:] only;
  "up2cat"   customunet.up2_cat: x, skip or None -> out; no parameters (decoder blocks 0, 1, 2 and 4);
  "up2into"  customunet.up2_into: x, buf -> buf IN PLACE (decoder block 3); no parameters.

The in-place edge: up2_into returns its ``buf`` argument, so the stem's output 0 and up2into's output 0 have the same storage, shape and
strides -- one key for the recorder.  The later call's entry replaces the earlier one, which is the right outcome: up2into's own ``buf``
input resolved (before its call) to the stem, and the consumer convolution resolves to up2into.  The wrapper asserts both instead of
leaving them to the order of a dict.

``_patch`` is a staticmethod bound when the class was created: patched on CustomUNetMI355X itself.
"""
import deeplabv3_nodes as N
from unet_nodes import _key

KINDS = ("patch", "conv", "bn", "stemskip", "up2cat", "up2into")
GRAD_SLOTS = {**{k: N.GRAD_SLOTS[k] for k in ("patch", "conv", "bn")}, "stemskip": {"y": 0, "gamma": 2, "beta": 3},
              "up2cat": {"x": 0, "skip": 1}, "up2into": {"x": 0, "buf": 1}}
DIFF_INPUTS = {**{k: N.DIFF_INPUTS[k] for k in ("patch", "conv", "bn")}, "stemskip": ("y",), "up2cat": ("x", "skip"), "up2into": ("x", "buf")}
PLACED = ("up2cat", "up2into")      # kinds whose call names no module: their place in the schedule identifies them


def schedule(model):
    """[(kind, name, module)] in the order CustomUNetMI355X._forward_native calls its nodes (the bf16 route)"""
    s = N.encoder_schedule(model)
    s.insert(1, ("stemskip", "encoder.bn1"))
    s = [(k, n, model.get_submodule(n)) for k, n in s]
    for i in range(5):
        s.append(("up2into" if i == 3 else "up2cat", f"decoder.blocks.{i}.up", None))
        for c in ("conv1", "conv2"):
            p = f"decoder.blocks.{i}.{c}"
            s += [("conv", f"{p}.0", model.get_submodule(f"{p}.0")), ("bn", f"{p}.1", model.get_submodule(f"{p}.1"))]
    s.append(("conv", "segmentation_head.0", model.get_submodule("segmentation_head.0")))
    return s


class Description(N.Description):
    label = "CustomUNetMI355X"
    kinds, grad_slots, diff_inputs = KINDS, GRAD_SLOTS, DIFF_INPUTS

    def schedule(self, model):
        return schedule(model)

    def norm_of(self, kind, module):
        return module if kind in ("bn", "stemskip") else None

    def params(self, node):
        if node.kind == "stemskip":
            return {"gamma": node.module.weight, "beta": node.module.bias}
        if node.kind in PLACED:
            return {}
        return super().params(node)

    def check_owner(self, kind, name, owner, module):
        if kind == "stemskip":
            assert owner is module, f"{name}: the call's module is not the model's {name}"
        elif kind not in PLACED:
            super().check_owner(kind, name, owner, module)

    def install(self, rec):
        from py4cast_amd import customunet as U

        cls = U.CustomUNetMI355X
        assert "_patch" in cls.__dict__, "CustomUNetMI355X binds its own _patch"
        rec.patch(cls, "_patch", staticmethod(rec.wrap_patch(cls._patch)))
        stem0, cat0, into0 = U.stem_tail_skip, U.up2_cat, U.up2_into

        def stem_tail_skip(y, stats, bn, offset):
            node = rec._begin("stemskip", bn, {"y": y, "stats": stats}, {"offset": int(offset)})
            buf, pool = stem0(y, stats, bn, offset)
            node.saved["arg"] = pool.grad_fn.saved_tensors[2].clone() if pool.grad_fn is not None else None
            rec._end(node, [buf, pool], pool.grad_fn)
            return buf, pool

        def up2_cat(x, skip):
            node = rec._begin("up2cat", None, {"x": x, "skip": skip}, {})
            out = cat0(x, skip)
            rec._end(node, [out], out.grad_fn)
            return out

        def up2_into(x, buf):
            # buf as the stem wrote it (its first channels uninitialised): cloned by _begin BEFORE the call fills them
            node = rec._begin("up2into", None, {"x": x, "buf": buf}, {})
            j, o = node.src.get("buf", (None, None))
            assert j is not None and rec.nodes[j].kind == "stemskip" and o == 0, "up2into's buf is not the stem's output 0"
            out = into0(x, buf)
            assert _key(out) == _key(buf), "up2_into no longer returns its buf argument"
            rec._end(node, [out], out.grad_fn)
            # the same key as the stem's output 0: from here on it names up2into's output
            assert rec._made[_key(out)] == (len(rec.nodes) - 1, 0)
            return out

        rec.patch(U, "stem_tail_skip", stem_tail_skip)
        rec.patch(U, "up2_cat", up2_cat)
        rec.patch(U, "up2_into", up2_into)
        for fn_cls in (U._StemTailSkip, U._Up2Cat, U._Up2Into):
            rec.wrap_backward(fn_cls)


def counts(model):
    return Description().counts(model)


def Recorder(model):
    return N.Recorder(model, Description())


def owned_parameters(model):
    """the ids of the parameters of every scheduled module (tests: each of the model's parameters exactly once)"""
    return [id(p) for _, _, mod in schedule(model) if mod is not None for p in mod.parameters()]
