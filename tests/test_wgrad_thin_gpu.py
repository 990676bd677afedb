"""
The thin weight-gradient kernel of the first convolution (csrc/conv_thin.hip: conv3x3_wgrad_thin_bf16_kernel): rows 64 .. C_in - 1 of dW
for 65..72 input channels on 96-channel pixels, against float64 on the SAME bf16-rounded operands, against the thin chunk of the
row-streaming kernel it replaces (P4C_WGRAD_THIN=0, diagnostic library), over the shapes that reach every path of its row loop (one strip
and a strip boundary; fewer rows than an interval, odd and even segment lengths; workgroup counts 1, 3 and more than there are segments),
with a closed-form border case for the zero-padding shifts, for reproducibility, for the shapes that must keep their route, and inside
one backward call of the plan.
"""
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("diag_library")]   # (flips P4C_* A/B switches: diagnostic build)

CIP, CO = 96, 64


def rel_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-30))


def _operands(dev, B, H, W, cin, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(B, H, W, CIP, generator=g, device=dev)
    x[..., cin:] = 0
    dy = torch.randn(B, H, W, 64, generator=g, device=dev)
    return x.bfloat16(), dy.bfloat16()


def _thin_rows_f64(x, dy, cin):
    """gw[co][c][ky][kx] for the channels 64 .. cin - 1 in float64 on the bf16 operands, "same" zero padding"""
    B, H, W, _ = x.shape
    xp = torch.nn.functional.pad(x[..., 64:cin].double(), (0, 0, 1, 1, 1, 1))
    ref = torch.zeros(CO, cin - 64, 3, 3, dtype=torch.float64, device=x.device)
    dyd = dy.double().reshape(-1, 64)
    for ky in range(3):
        for kx in range(3):
            ref[:, :, ky, kx] = dyd.t() @ xp[:, ky:ky + H, kx:kx + W, :].reshape(-1, cin - 64)
    return ref


def _wgrad(monkeypatch, x, dy, cin, thin, nwg=None, compute="bf16"):
    from py4cast_amd import ops_model as om

    monkeypatch.setenv("P4C_WGRAD_THIN", "1" if thin else "0")
    if nwg is None:
        monkeypatch.delenv("P4C_WGRAD_THIN_G", raising=False)
    else:
        monkeypatch.setenv("P4C_WGRAD_THIN_G", str(nwg))
    grad = torch.zeros(CO, cin, 3, 3, device=x.device)
    return om.conv_wgrad(x, dy, 3, CO, cin, grad, compute=compute)


# B, H, W, C_in, workgroups (None: the launcher's choice).  W = 64: one strip, W = 128: the column halo comes from the neighbouring strip;
# H = 1, 2, 3: at most one interval and a half; 7, 33: odd segments; 32: even; workgroups 1 / 3: a workgroup walks several (sample,
# strip, segment) items; 1000: more than there are rows -- one-row segments, the count clamped to the items
CASES = [
    (1, 1, 64, 69, None),
    (1, 2, 64, 65, 1),
    (2, 3, 64, 72, 3),
    (2, 1, 128, 72, 1000),
    (1, 2, 128, 69, 3),
    (1, 3, 128, 69, 1),
    (1, 7, 64, 69, 1000),
    (2, 7, 128, 65, 3),
    (2, 7, 128, 72, None),
    (1, 32, 64, 72, 1),
    (2, 32, 128, 69, None),
    (2, 32, 128, 65, 1000),
    (2, 33, 64, 69, 1000),
    (1, 33, 128, 65, 3),
    (2, 33, 128, 72, 1),
    (2, 33, 128, 69, 24),
]


@pytest.mark.parametrize("B,H,W,cin,nwg", CASES)
def test_thin_wgrad_vs_float64_and_the_thin_chunk(gpu_device, monkeypatch, B, H, W, cin, nwg):
    x, dy = _operands(gpu_device, B, H, W, cin, 1000 * B + 10 * H + cin)
    ref = _thin_rows_f64(x, dy, cin)
    new = _wgrad(monkeypatch, x, dy, cin, True, nwg)
    old = _wgrad(monkeypatch, x, dy, cin, False)
    e64, eold = rel_err(new[:, 64:], ref), rel_err(new[:, 64:], old[:, 64:])
    print(f"thin rows: vs float64 {e64:.3e}, vs the thin chunk {eold:.3e}")
    assert e64 < 5e-4, e64                               # the project's bar for weight gradients
    assert eold < 5e-5, eold                             # a kernel replacing a kernel: the same products, fp32 sums in another order
    assert torch.equal(new[:, :64], old[:, :64])         # the full chunk is launched exactly as before


@pytest.mark.parametrize("cin", [65, 69])
def test_rows_beyond_the_real_channels_are_exactly_zero(gpu_device, monkeypatch, cin):
    """the octet's channels beyond C_in are zero padding of x: declared as real (C_in = 72) their gradient rows are sums of zeros, so
    no row of the 72-row product leaks into another; declared as they are, the result has C_in rows and is the same"""
    x, dy = _operands(gpu_device, 2, 7, 128, cin, cin)
    wide = _wgrad(monkeypatch, x, dy, 72, True, 3)
    assert bool((wide[:, cin:] == 0).all())
    assert torch.equal(wide[:, :cin], _wgrad(monkeypatch, x, dy, cin, True, 3))


@pytest.mark.parametrize("B,H,W,nwg", [(2, 7, 128, 3), (1, 33, 64, None), (1, 2, 128, 1)])
def test_border_pixels_closed_form(gpu_device, monkeypatch, B, H, W, nwg):
    """x = c + 1 in thin channel c on the image border and 0 inside, dY = 1: dW[co][64 + c][ky][kx] = B (c + 1) x the number of border
    pixels whose tap partner lies inside the image -- small integers, exact in bf16 and fp32; a wrong zero-padding shift changes them"""
    cin = 72
    x = torch.zeros(B, H, W, CIP, device=gpu_device)
    edge = torch.zeros(H, W, dtype=torch.bool, device=gpu_device)
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
    x[:, edge, 64:72] = torch.arange(1, 9, device=gpu_device, dtype=torch.float32)
    dy = torch.ones(B, H, W, 64, device=gpu_device)
    got = _wgrad(monkeypatch, x.bfloat16(), dy.bfloat16(), cin, True, nwg)[:, 64:]
    border = 2 * W + 2 * H - 4
    for ky in range(3):
        for kx in range(3):
            ay, ax = abs(ky - 1), abs(kx - 1)
            count = border - (ay * W + ax * H - ay * ax)      # x pixel (u, v) meets dY pixel (u - ky + 1, v - kx + 1), if that exists
            want = B * count * torch.arange(1, 9, device=gpu_device, dtype=torch.float32)
            assert torch.equal(got[:, :, ky, kx], want.expand(CO, 8)), (ky, kx)


def test_thin_wgrad_is_reproducible(gpu_device, monkeypatch):
    x, dy = _operands(gpu_device, 2, 33, 128, 69, 5)
    for nwg in (None, 3):
        assert torch.equal(_wgrad(monkeypatch, x, dy, 69, True, nwg), _wgrad(monkeypatch, x, dy, 69, True, nwg))


@pytest.mark.parametrize("what", ["cin64", "cin80", "w96", "f32"])
def test_other_shapes_keep_their_route(gpu_device, monkeypatch, what):
    """64 and 80 input channels, a map that is no multiple of the strip wide, the fp32 flavour: the switch changes nothing"""
    from py4cast_amd import ops_model as om

    cin, cip, W, dt, compute = {"cin64": (64, 64, 128, torch.bfloat16, "bf16"), "cin80": (80, 96, 128, torch.bfloat16, "bf16"),
                                "w96": (69, 96, 96, torch.bfloat16, "bf16"), "f32": (69, 96, 128, torch.float32, "f32")}[what]
    g = torch.Generator(device=gpu_device).manual_seed(7)
    x = torch.randn(2, 16, W, cip, generator=g, device=gpu_device)
    x[..., cin:] = 0
    x, dy = x.to(dt), torch.randn(2, 16, W, 64, generator=g, device=gpu_device).to(dt)
    res = []
    for sw in ("1", "0"):
        monkeypatch.setenv("P4C_WGRAD_THIN", sw)
        res.append(om.conv_wgrad(x, dy, 3, CO, cin, torch.zeros(CO, cin, 3, 3, device=gpu_device), compute=compute))
    assert torch.equal(res[0], res[1])
    assert float(res[0].abs().max()) > 0


def test_plan_backward_with_and_without_the_thin_kernel(gpu_device, monkeypatch):
    """one p4c_halfunet_backward call at B = 1, 64 x 64, 69 inputs: the thin job's compact slabs are reduced by the call's ONE batched
    reduction beside the full chunk's job.  Reruns are bit-identical; against the switch off every gradient is bit-equal except rows
    64..68 of the first convolution's, which differ by the order of their fp32 sums"""
    from py4cast_amd.halfunet import HalfUNetMI355X, HalfUNetSettings

    torch.manual_seed(2)
    model = HalfUNetMI355X(69, 60, (64, 64), HalfUNetSettings(compute_dtype="bf16", activation_dtype="bf16")).to(gpu_device).train()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 64, 64, 69, generator=g).to(gpu_device)
    gy = torch.randn(1, 64, 64, 60, generator=g).to(gpu_device)
    first = [n for n, p in model.named_parameters() if tuple(p.shape) == (64, 69, 3, 3)]
    assert len(first) == 1

    def run(thin):
        monkeypatch.setenv("P4C_WGRAD_THIN", "1" if thin else "0")
        model.zero_grad(set_to_none=True)
        xg = x.clone().requires_grad_(True)
        y = model(xg)
        (y * gy).sum().backward()
        torch.cuda.synchronize()
        return y.detach().clone(), xg.grad.clone(), {n: p.grad.clone() for n, p in model.named_parameters()}

    ya, dxa, ga = run(True)
    yb, dxb, gb = run(True)
    assert torch.equal(ya, yb) and torch.equal(dxa, dxb) and all(torch.equal(ga[n], gb[n]) for n in ga)
    yo, dxo, go = run(False)
    assert torch.equal(ya, yo) and torch.equal(dxa, dxo)
    for n in ga:
        if n == first[0]:
            assert torch.equal(ga[n][:, :64], go[n][:, :64])
            e = rel_err(ga[n][:, 64:], go[n][:, 64:])
            print(f"dW0 rows 64..68, thin kernel vs thin chunk: {e:.3e}")
            assert e < 5e-5, e
        else:
            assert torch.equal(ga[n], go[n]), n
