"""csrc/conv_chain.hip, the ring kernel's forms (conv_chain_ring_kernel, variant 2; persistent for the dual
layer1 boundary, one tile per block with 2 or 3 stages for layer2): every
instantiation must compute y and t1 bit for bit as the one-tile-per-block kernel (variant 1) does,
and stay within tests/test_chain_gpu.py's tolerances of the fp32 reference.

Shapes: the smallest at which the new code can go wrong -- a single ragged tile, blocks that take
unequal tile counts (the cross-tile prefetch runs past a block's last tile), a block with no tile at
all, and M tails on the layer2 shapes."""
import functools

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


def _run(variant, grid, fn):
    from mlmicroservicetemplate_amd import ops

    lib = ops.lib()
    try:
        lib.mls_chain_set_variant(variant)
        lib.mls_chain_set_grid(grid)
        out = fn()
        torch.cuda.synchronize()
        return out
    finally:
        lib.mls_chain_set_variant(0)
        lib.mls_chain_set_grid(0)


@functools.lru_cache(maxsize=None)
def _residual_case(shape):
    """Inputs, the variant-1 outputs and the fp32 reference of one residual-form boundary (computed once)."""
    from mlmicroservicetemplate_amd import ops

    B, H, K, N1, N2 = shape
    torch.manual_seed(sum(shape))
    t2 = torch.relu(_rand(B, H, H, K))
    res = _rand(B, H, H, N1)
    w3 = _rand(N1, K, scale=K**-0.5)
    w1 = _rand(N2, N1, scale=N1**-0.5)
    b3, b1 = torch.randn(N1, device=DEV) * 0.1, torch.randn(N2, device=DEV) * 0.1
    call = lambda: ops.conv1x1_chain(t2, w3, b3, w1, b1, residual=res)  # noqa: E731
    y1, t11 = _run(1, 0, call)
    y_ref = torch.relu(t2.float() @ w3.float().T + b3 + res.float())
    t1_ref = torch.relu(y_ref.to(torch.bfloat16).float() @ w1.float().T + b1)
    return call, y1, t11, y_ref, t1_ref


@functools.lru_cache(maxsize=None)
def _dual_case(stride2, H2, B):
    from mlmicroservicetemplate_amd import ops

    Ka, Kb, N1, N2 = 64, 64, 256, 64
    Ho = (H2 - 1) // stride2 + 1
    torch.manual_seed(stride2 + H2)
    t2 = torch.relu(_rand(B, Ho, Ho, Ka))
    x = _rand(B, H2, H2, Kb)
    w3 = _rand(N1, Ka, scale=Ka**-0.5)
    wd = _rand(N1, Kb, scale=Kb**-0.5)
    w1 = _rand(N2, N1, scale=N1**-0.5)
    b3, b1 = torch.randn(N1, device=DEV) * 0.1, torch.randn(N2, device=DEV) * 0.1
    wcat = torch.cat([w3, wd], 1).contiguous()
    call = lambda: ops.conv1x1_chain(t2, wcat, b3, w1, b1, a2=x, stride2=stride2)  # noqa: E731
    y1, t11 = _run(1, 0, call)
    xs = x[:, ::stride2, ::stride2, :][:, :Ho, :Ho, :]
    y_ref = torch.relu(t2.float() @ w3.float().T + xs.float() @ wd.float().T + b3)
    t1_ref = torch.relu(y_ref.to(torch.bfloat16).float() @ w1.float().T + b1)
    return call, y1, t11, y_ref, t1_ref


def _check(case, grid):
    call, y1, t11, y_ref, t1_ref = case
    y2, t12 = _run(2, grid, call)
    assert torch.equal(y2, y1) and torch.equal(t12, t11)
    assert rel_err(y2, y_ref) < 1e-2 and rel_err(t12, t1_ref) < 2e-2


# the persistent stage-opening (dual) form, 64-row tiles.  M = 49: one ragged tile, and a grid of 3
# leaves two blocks without a tile; M = 1568 (stride 1): 25 tiles, which grids of 4 and 5 split
# unequally or run the prefetch past every block's last tile; M = 162 (stride 2): 3 tiles, the last
# ragged, fewer than either grid
@pytest.mark.parametrize("stride2,H2,B,grid", [(1, 7, 1, 1), (1, 7, 1, 3), (1, 28, 2, 4), (1, 28, 2, 5), (1, 28, 2, 0),
                                               (2, 17, 2, 4), (2, 17, 2, 5), (2, 17, 2, 0)])
def test_persistent_dual_matches_one_tile_per_block(stride2, H2, B, grid):
    _check(_dual_case(stride2, H2, B), grid)


# dispatch only: the single-slab layer1 boundaries have no ring instantiation (none measured faster),
# so variant 2 must run conv_chain_kernel for them, not refuse them
@pytest.mark.parametrize("shape", [(2, 28, 64, 256, 64), (2, 28, 64, 256, 128)], ids=lambda s: "x".join(map(str, s)))
def test_variant2_falls_back_where_nothing_is_instantiated(shape):
    _check(_residual_case(shape), 0)


# layer2, one tile per block: N2 = 128 keeps the 2 stages of 64 channels (only the epilogue's LDS accesses
# differ from conv_chain_kernel), N2 = 256 runs 3 stages of 32 channels, which exercises the counted wait's
# tail (fewer stages left than ring slots).  M = 243 and 392: ragged last tiles
@pytest.mark.parametrize("shape", [(3, 9, 128, 512, 128), (2, 14, 128, 512, 256)],
                         ids=lambda s: "x".join(map(str, s)))
def test_layer2_ring_matches_one_tile_per_block(shape):
    _check(_residual_case(shape), 0)


def test_resnet50_logits_equal_across_variants():
    from mlmicroservicetemplate_amd.models.resnet import ResNet50Fused, init_resnet50

    params = init_resnet50(0)
    torch.manual_seed(5)
    imgs = torch.randint(0, 256, (4, 224, 224, 3), dtype=torch.uint8, device=DEV)
    model = ResNet50Fused(params, DEV, max_batch=4)
    assert model.chain
    old = _run(1, 0, lambda: model(imgs).clone())
    new = _run(2, 0, lambda: model(imgs).clone())
    assert torch.equal(new, old)
