"""csrc/conv_chain.hip, the Y2 store (``y_stride2=True``): at a stage boundary in front of a stride-2
dual block the kernel keeps only the pixels (2i, 2j) of the block output y, compactly as
[B][Ho/2][Wo/2][N1]; t1 (the next block's conv1 output, computed from all of y in LDS) is untouched.

Per supported form -- (1, 256, 128) plain and with conv2 fused, (2, 512, 256) in conv_chain_kernel
(variant 1) and in the ring kernel (variant 2) -- the compact y must be the full store's
``y[:, ::2, ::2, :]`` bit for bit (the kept pixels are the same registers going to another address),
t1 must not change by a bit, both stay within the fp32 tolerance tests/test_chain_gpu.py holds these
ops to (the reference is the same plain-PyTorch fp32 computation those tests use), and nothing
outside the compact window is written.  Shapes: one full 128-row tile plus a tail with image ends
inside a tile (3x8x8), a single partial tile with Ho != Wo (2x6x10), several tiles with image rows
straddling tile edges (5x12x12)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 12288.0  # exact in bf16, far outside the values the ops produce here
PAD = 4096  # sentinel elements on each side of the compact y window


@pytest.fixture(scope="module", autouse=True)
def _native():
    from mlmicroservicetemplate_amd import ops

    ops.lib()
    yield
    ops.lib().mls_chain_set_variant(0)


def rel_err(a, b):
    return ((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-6)).item()


def _rand(*shape, scale=1.0):
    return (torch.randn(*shape, device=DEV) * scale).to(torch.bfloat16)


# form -> (Ka, N1, N2, conv2 fused, mls_chain_set_variant)
FORMS = {"l1_plain": (64, 256, 128, False, 0), "l1_conv2": (64, 256, 128, True, 0),
         "l2_chain": (128, 512, 256, False, 1), "l2_ring": (128, 512, 256, False, 2)}
SHAPES = [(3, 8, 8), (2, 6, 10), (5, 12, 12)]


def _case(form, shape):
    Ka, N1, N2, c2, _v = FORMS[form]
    B, H, W = shape
    torch.manual_seed(B * 1000 + H * 10 + W + N2)
    c = {"a": torch.relu(_rand(B, H, W, Ka)), "res": _rand(B, H, W, N1), "w3": _rand(N1, Ka, scale=Ka**-0.5),
         "b3": torch.randn(N1, device=DEV) * 0.1, "w1": _rand(N2, N1, scale=N1**-0.5),
         "b1": torch.randn(N2, device=DEV) * 0.1}
    if c2:  # a is the conv2 input t1_in
        c["w2"], c["b2"] = _rand(64, 3, 3, 64, scale=(9 * 64) ** -0.5), torch.randn(64, device=DEV) * 0.1
    return c


def _run(ops, form, c, **kw):
    if FORMS[form][3]:
        return ops.conv3x3_chain(c["a"], c["w2"], c["b2"], c["w3"], c["b3"], c["w1"], c["b1"], residual=c["res"], **kw)
    return ops.conv1x1_chain(c["a"], c["w3"], c["b3"], c["w1"], c["b1"], residual=c["res"], **kw)


def _reference(form, c):
    """fp32 on the bf16 inputs; t2 and y rounded to bf16 where the network rounds them."""
    t2 = c["a"].float()
    if FORMS[form][3]:
        t2 = torch.nn.functional.conv2d(t2.permute(0, 3, 1, 2), c["w2"].float().permute(0, 3, 1, 2), c["b2"], padding=1)
        t2 = torch.relu(t2).permute(0, 2, 3, 1).to(torch.bfloat16).float()
    y = torch.relu(t2 @ c["w3"].float().T + c["b3"] + c["res"].float())
    return y, torch.relu(y.to(torch.bfloat16).float() @ c["w1"].float().T + c["b1"])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("form", list(FORMS))
def test_compact_y_is_the_full_store_subsampled(form, shape):
    from mlmicroservicetemplate_amd import ops

    B, H, W = shape
    N1 = FORMS[form][1]
    c = _case(form, shape)
    n = B * (H // 2) * (W // 2) * N1
    buf = torch.full((n + 2 * PAD,), SENTINEL, device=DEV, dtype=torch.bfloat16)
    window = buf[PAD:PAD + n].view(B, H // 2, W // 2, N1)
    ops.lib().mls_chain_set_variant(FORMS[form][4])
    try:
        y_full, t1_full = _run(ops, form, c)
        y, t1 = _run(ops, form, c, y_stride2=True, y_out=window)
    finally:
        ops.lib().mls_chain_set_variant(0)
    assert y.data_ptr() == window.data_ptr() and tuple(y.shape) == (B, H // 2, W // 2, N1)
    assert torch.equal(y, y_full[:, ::2, ::2, :])
    assert torch.equal(t1, t1_full)
    y_ref, t1_ref = _reference(form, c)
    e = (rel_err(y, y_ref[:, ::2, ::2, :]), rel_err(y_full, y_ref), rel_err(t1, t1_ref))
    print(f"{form} {shape}: vs fp32 compact y {e[0]:.2e} full y {e[1]:.2e} t1 {e[2]:.2e}")
    assert e[0] < 1e-2 and e[1] < 1e-2 and e[2] < 2e-2
    assert (buf[:PAD] == SENTINEL).all() and (buf[PAD + n:] == SENTINEL).all()


def test_compact_y_allocated_by_the_op():
    from mlmicroservicetemplate_amd import ops

    c = _case("l1_plain", (2, 6, 10))
    y_full, _ = _run(ops, "l1_plain", c)
    y, _ = _run(ops, "l1_plain", c, y_stride2=True)
    assert tuple(y.shape) == (2, 3, 5, 256) and torch.equal(y, y_full[:, ::2, ::2, :])


@pytest.mark.parametrize("form,shape", [("l1_plain", (2, 7, 8)), ("l1_plain", (2, 8, 7)), ("l1_conv2", (2, 7, 8)),
                                        ("l2_chain", (2, 8, 9))])
def test_odd_grid_is_rejected_before_a_launch(form, shape):
    """Odd Ho or Wo: the Python op raises, and the C entry point returns an error with y and t1 untouched."""
    from mlmicroservicetemplate_amd import ops

    B, H, W = shape
    Ka, N1, N2, c2, _v = FORMS[form]
    c = _case(form, shape)
    with pytest.raises(ValueError):
        _run(ops, form, c, y_stride2=True)
    y = torch.full((B, H, W, N1), SENTINEL, device=DEV, dtype=torch.bfloat16)
    t1 = torch.full((B, H, W, N2), SENTINEL, device=DEV, dtype=torch.bfloat16)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()  # noqa: E731
    if c2:
        rc = ops.lib().mls_conv_chain_conv2_y2(p(c["a"]), p(c["w2"]), p(c["b2"]), None, p(c["w3"]), p(c["b3"]),
                                               p(c["res"]), p(y), p(c["w1"]), p(c["b1"]), p(t1), B, H, W, 64, 0, 0, 0, 1,
                                               N1, N2, st)
    else:
        rc = ops.lib().mls_conv_chain_y2(p(c["a"]), None, p(c["w3"]), p(c["b3"]), p(c["res"]), p(y), p(c["w1"]),
                                         p(c["b1"]), p(t1), B, H, W, Ka, 0, 0, 0, 1, N1, N2, st)
    torch.cuda.synchronize()
    assert rc != 0
    assert (y == SENTINEL).all() and (t1 == SENTINEL).all()


def test_shapes_without_the_form_are_rejected_before_a_launch():
    """A boundary that is not in front of a stride-2 stage has no Y2 instantiation."""
    from mlmicroservicetemplate_amd import ops

    B, H, W, Ka, N1, N2 = 2, 8, 8, 128, 512, 128  # layer2.1 -> 2.2
    a, res = torch.relu(_rand(B, H, W, Ka)), _rand(B, H, W, N1)
    w3, w1 = _rand(N1, Ka, scale=Ka**-0.5), _rand(N2, N1, scale=N1**-0.5)
    with pytest.raises(ValueError):
        ops.conv1x1_chain(a, w3, None, w1, None, residual=res, y_stride2=True)
    y = torch.full((B, H, W, N1), SENTINEL, device=DEV, dtype=torch.bfloat16)
    t1 = torch.full((B, H, W, N2), SENTINEL, device=DEV, dtype=torch.bfloat16)
    st = torch.cuda.current_stream().cuda_stream
    rc = ops.lib().mls_conv_chain_y2(a.data_ptr(), None, w3.data_ptr(), None, res.data_ptr(), y.data_ptr(),
                                     w1.data_ptr(), None, t1.data_ptr(), B, H, W, Ka, 0, 0, 0, 1, N1, N2, st)
    torch.cuda.synchronize()
    assert rc != 0
    assert (y == SENTINEL).all() and (t1 == SENTINEL).all()
    c = _case("l1_conv2", (2, 8, 8))  # conv2 fused, N2 = 64: layer1.1 -> 1.2
    with pytest.raises(ValueError):
        ops.conv3x3_chain(c["a"], c["w2"], c["b2"], c["w3"], c["b3"], _rand(64, 256), None, residual=c["res"],
                          y_stride2=True)


def test_resnet50_logits_identical_with_and_without_the_compact_store():
    """ResNet50Fused at B = 2: both stage boundaries take the compact store (and the layer1 one also in
    its conv2-fused form), the dual blocks behind them read it at stride 1, and the logits do not
    change by a bit against the full store."""
    from mlmicroservicetemplate_amd.models.resnet import CHAIN_CONV2_DEFAULT, ResNet50Fused, init_resnet50

    params = init_resnet50(0)
    torch.manual_seed(13)
    imgs = torch.randint(0, 256, (2, 224, 224, 3), dtype=torch.uint8, device=DEV)
    model = ResNet50Fused(params, DEV, max_batch=2)
    ops = model.ops
    seen = []
    real = {"conv1x1_chain": ops.conv1x1_chain, "conv3x3_chain": ops.conv3x3_chain}

    def spy(name):
        def f(*a, **k):
            y, t1 = real[name](*a, **k)
            if k.get("y_stride2"):
                seen.append((name, tuple(y.shape)))
            return y, t1
        return f

    ops.conv1x1_chain, ops.conv3x3_chain = spy("conv1x1_chain"), spy("conv3x3_chain")
    try:
        out = {}
        for conv2_all in (False, True):
            model.chain_conv2 = True
            model.chain_conv2_shapes = ops.CHAIN_CONV2_SHAPES if conv2_all else CHAIN_CONV2_DEFAULT
            for on in (True, False):
                model.chain_y_stride2 = on
                out[conv2_all, on] = model(imgs).clone()
    finally:
        ops.conv1x1_chain, ops.conv3x3_chain = real["conv1x1_chain"], real["conv3x3_chain"]
    assert seen == [("conv1x1_chain", (2, 28, 28, 256)), ("conv1x1_chain", (2, 14, 14, 512)),
                    ("conv3x3_chain", (2, 28, 28, 256)), ("conv1x1_chain", (2, 14, 14, 512))]
    assert torch.equal(out[False, True], out[False, False])
    assert torch.equal(out[True, True], out[True, False])
