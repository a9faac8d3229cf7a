"""csrc/conv_chain.hip, the C2 form (ops.conv3x3_chain): a bottleneck's 3x3 conv2 computed inside the
chained boundary kernel -- t2 = relu(conv3x3(t1) + b2) goes straight into the chain's A-tile LDS
image and never to memory -- vs a plain-PyTorch fp32 reference and vs the two launches it replaces
(the 3x3 conv kernel, then ops.conv1x1_chain).

The tile is 128 rows of the flattened [B*H*W] pixel list, so tiles cross image rows and images; the
shapes below put two image ends inside one tile, a partial last tile, a halo (W + 1) longer than a
row, a non-square image and the workload's 56x56 with an image boundary in the middle of a tile."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _native():
    from mlmicroservicetemplate_amd import ops

    ops.lib()
    yield


def rel_err(a, b):
    return ((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-6)).item()


def _rand(*shape, scale=1.0):
    return (torch.randn(*shape, device=DEV) * scale).to(torch.bfloat16)


def _case(B, H, W, Kb, N1, N2, seed):
    """Inputs of one boundary: t1, conv2, conv3 (+ residual, or + the dual operand x at stride 1), conv1."""
    torch.manual_seed(seed)
    c = {"t1": torch.relu(_rand(B, H, W, 64)), "w2": _rand(64, 3, 3, 64, scale=(9 * 64) ** -0.5),
         "b2": torch.randn(64, device=DEV) * 0.1, "w3": _rand(N1, 64 + Kb, scale=(64 + Kb) ** -0.5),
         "b3": torch.randn(N1, device=DEV) * 0.1, "w1": _rand(N2, N1, scale=N1**-0.5),
         "b1": torch.randn(N2, device=DEV) * 0.1}
    c["res"] = _rand(B, H, W, N1) if Kb == 0 else None
    c["x"] = _rand(B, H, W, Kb) if Kb else None
    return c


def _fused(ops, c):
    return ops.conv3x3_chain(c["t1"], c["w2"], c["b2"], c["w3"], c["b3"], c["w1"], c["b1"], residual=c["res"],
                             a2=c["x"], stride2=1)


def _unfused(ops, c):
    """The two launches: conv2 on the pipelined 3x3 kernel (the implicit-GEMM conv where that kernel
    has no geometry for the shape), then the chain."""
    B, H, W, _ = c["t1"].shape
    if ops.conv3x3_pipe_geometry(B, H, W) is not None:
        t2 = ops.conv3x3_pipe(c["t1"], c["w2"], c["b2"], act=ops.ACT_RELU)
    else:
        t2 = ops.conv2d_nhwc(c["t1"], c["w2"], c["b2"], kernel=3, stride=1, pad=1, act=ops.ACT_RELU)
    return ops.conv1x1_chain(t2, c["w3"], c["b3"], c["w1"], c["b1"], residual=c["res"], a2=c["x"], stride2=1)


def _reference(c):
    """fp32 on the bf16 inputs; t2 and y rounded to bf16 where the network rounds them."""
    t2 = torch.nn.functional.conv2d(c["t1"].float().permute(0, 3, 1, 2), c["w2"].float().permute(0, 3, 1, 2),
                                    c["b2"], padding=1)
    t2 = torch.relu(t2).permute(0, 2, 3, 1).to(torch.bfloat16).float()
    y = t2 @ c["w3"][:, :64].float().T + c["b3"]
    if c["x"] is not None:
        y = y + c["x"].float() @ c["w3"][:, 64:].float().T
    if c["res"] is not None:
        y = y + c["res"].float()
    y = torch.relu(y)
    t1n = torch.relu(y.to(torch.bfloat16).float() @ c["w1"].float().T + c["b1"])
    return y, t1n


def _check(shape, Kb, N1, N2):
    from mlmicroservicetemplate_amd import ops

    B, H, W = shape
    c = _case(B, H, W, Kb, N1, N2, seed=B * 1000 + H * 10 + W + N2 + Kb)
    y, t1n = _fused(ops, c)
    y_ref, t1n_ref = _reference(c)
    e = (rel_err(y, y_ref), rel_err(t1n, t1n_ref))
    y_u, t1n_u = _unfused(ops, c)
    eu = (rel_err(y, y_u), rel_err(t1n, t1n_u))
    print(f"conv3x3_chain {shape} Kb={Kb} N2={N2}: vs fp32 y {e[0]:.2e} t1 {e[1]:.2e}; "
          f"vs unfused y {eu[0]:.2e} t1 {eu[1]:.2e}")
    assert e[0] < 1e-2 and e[1] < 2e-2
    assert eu[0] < 1e-2 and eu[1] < 1e-2


SHAPES = [(3, 9, 9), (2, 5, 12), (1, 56, 56), (2, 56, 56)]


@pytest.mark.parametrize("n2", [64, 128])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv2_chain_residual(shape, n2):
    """(KS, N1, N2) = (1, 256, 64) and (1, 256, 128): layer1.1 -> 1.2 and layer1.2 -> layer2.0."""
    _check(shape, 0, 256, n2)


@pytest.mark.parametrize("shape", [(3, 9, 9), (2, 56, 56)], ids=lambda s: "x".join(map(str, s)))
def test_conv2_chain_dual(shape):
    """(2, 256, 64): layer1.0 -> 1.1, [t2 | x] at stride 1; only the t2 slab is computed."""
    _check(shape, 64, 256, 64)


@pytest.mark.parametrize("shape", [(3, 9, 9), (2, 5, 12), (1, 56, 56)], ids=lambda s: "x".join(map(str, s)))
def test_conv2_chain_border_taps_exact(shape):
    """All-ones t1 and W2, zero bias, W3 = identity on the first 64 channels, no residual: y[..., :64]
    is 64 x the number of in-image taps of the pixel (4 corner / 6 edge / 9 interior), exactly
    representable in bf16, so a wrong border mask is an exact integer error."""
    from mlmicroservicetemplate_amd import ops

    B, H, W = shape
    t1 = torch.ones(B, H, W, 64, device=DEV, dtype=torch.bfloat16)
    w2 = torch.ones(64, 3, 3, 64, device=DEV, dtype=torch.bfloat16)
    w3 = torch.zeros(256, 64, device=DEV, dtype=torch.bfloat16)
    w3[:64] = torch.eye(64, device=DEV, dtype=torch.bfloat16)
    w1 = torch.zeros(64, 256, device=DEV, dtype=torch.bfloat16)
    y, t1n = ops.conv3x3_chain(t1, w2, None, w3, None, w1, None)
    ny = 3 - (torch.arange(H) == 0).int() - (torch.arange(H) == H - 1).int()
    nx = 3 - (torch.arange(W) == 0).int() - (torch.arange(W) == W - 1).int()
    taps = (ny.view(H, 1) * nx.view(1, W)).to(DEV).float()  # in-image taps per pixel
    want = (64.0 * taps).view(1, H, W, 1).expand(B, H, W, 64)
    assert torch.equal(y[..., :64].float(), want)
    assert not y[..., 64:].any() and not t1n.any()


def test_conv2_chain_rejects_unsupported():
    from mlmicroservicetemplate_amd import ops

    c = _case(1, 4, 64, 0, 256, 64, seed=1)  # W = 64: the strip with its halo does not fit 256 rows
    with pytest.raises(ValueError):
        _fused(ops, c)
    c = _case(1, 7, 7, 0, 512, 128, seed=2)  # not a layer1 boundary
    with pytest.raises(ValueError):
        _fused(ops, c)


def test_resnet50_conv2_fused_matches_two_launches():
    """The network with conv2 inside the layer1 boundary kernels computes what it computes with conv2 as
    its own launch, within the bound tests/test_engine_gpu.py holds the logits to against fp32."""
    from mlmicroservicetemplate_amd.models.resnet import ResNet50Fused, init_resnet50, resnet50_reference

    params = init_resnet50(0)
    torch.manual_seed(11)
    imgs = torch.randint(0, 256, (2, 224, 224, 3), dtype=torch.uint8, device=DEV)
    model = ResNet50Fused(params, DEV, max_batch=2)
    calls = []
    real = model.ops.conv3x3_chain

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)

    model.chain_conv2, model.chain_conv2_shapes = True, model.ops.CHAIN_CONV2_SHAPES  # all three boundaries
    model.ops.conv3x3_chain = counting
    try:
        fused = model(imgs).float()
    finally:
        model.ops.conv3x3_chain = real
    assert len(calls) == 3  # layer1.0, layer1.1, layer1.2
    model.chain_conv2 = False
    plain = model(imgs).float()
    ref = resnet50_reference({k: v.to(DEV) for k, v in params.items()}, imgs)
    print(f"logits fused vs two launches {rel_err(fused, plain):.2e}; vs fp32 {rel_err(fused, ref):.2e}")
    assert rel_err(fused, plain) < 2e-2
    assert rel_err(fused, ref) < 2e-2
