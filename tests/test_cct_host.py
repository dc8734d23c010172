"""CPU: CCT's public interface, module tree, state_dict contract, seeded init and refused configurations against the reference
fixture (tests/golden/cct_small.npz), the fp32 restatement tests/cct_ref.py against the reference's logits, loss and gradients
(the dropout case with the recorded masks), and the new C-ABI prototypes with their shape / pointer answers.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cct_fixture as CF
import cct_ref as R
import port_checks as PC
from noise_robust_vit_amd import cct as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "cct_small.npz")
NEW = ["nrv_relu_maxpool_fwd", "nrv_relu_maxpool_bwd", "nrv_layernorm_f32_fwd", "nrv_layernorm_f32_bwd_workspace",
       "nrv_layernorm_f32_bwd", "nrv_seqpool_fwd", "nrv_seqpool_bwd_workspace", "nrv_seqpool_bwd"]
ERR_NULL, ERR_SHAPE, ERR_DTYPE, ERR_WORKSPACE, ERR_ALIGN = -1, -2, -3, -4, -5


@pytest.fixture(scope="module")
def fx():
    return np.load(FIX)


@pytest.fixture(scope="module")
def lib():
    from noise_robust_vit_amd import _lib, build
    return _lib.bind(build.build())


def test_public_interface():
    import noise_robust_vit_amd as pkg
    assert pkg.CCT is V.CCT and pkg.cct is V and "CCT" in pkg.__all__ and "cct" in pkg.__all__
    for name in ("cct_2", "cct_4", "cct_6", "cct_7", "cct_8", "cct_14", "cct_16", "CCT", "Tokenizer", "TransformerClassifier",
                 "TransformerEncoderLayer", "Attention", "DropPath", "sinusoidal_embedding"):
        assert name in V.__all__ and hasattr(V, name), name
    for fn, (L, H, r, D) in {"cct_2": (2, 2, 1, 128), "cct_4": (4, 2, 1, 128), "cct_6": (6, 4, 2, 256), "cct_7": (7, 4, 2, 256),
                             "cct_8": (8, 4, 2, 256), "cct_14": (14, 6, 3, 384), "cct_16": (16, 6, 3, 384)}.items():
        if L > 8:
            continue                                                        # the large builders: construction only costs time
        m = getattr(V, fn)(img_size=32, n_conv_layers=1, num_classes=10)
        c = m.classifier
        assert len(c.blocks) == L and c.blocks[0].self_attn.heads == H and c.embedding_dim == D
        assert c.blocks[0].linear1.out_features == D * r and c.sequence_length == 256
        # _cct's defaults: kernel 3 -> stride max(1, 3 // 2 - 1) = 1, padding max(1, 3 // 2) = 1
        conv = m.tokenizer.conv_layers[0][0]
        assert conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1) and conv.bias is None
    m = V.cct_2(img_size=32, robust=True, attention_dropout=0.0, stochastic_depth_rate=0.3)
    assert all(b.self_attn.robust and b._meta.robust and b.self_attn.attn_drop.p == 0.0 for b in m.classifier.blocks)
    assert [round(b.drop_path.drop_prob, 6) for b in m.classifier.blocks] == [0.0, 0.3]
    assert [b._site for b in m.classifier.blocks] == [-2, -3] and m.grad_groups() == []
    d = V.CCT(img_size=16, embedding_dim=64, num_layers=2, num_heads=2)
    assert not any(b.self_attn.robust for b in d.classifier.blocks)
    assert all(b.self_attn.attn_drop.p == 0.1 for b in d.classifier.blocks)           # the reference's hard-wired 0.1
    assert [round(b.drop_path.drop_prob, 6) for b in d.classifier.blocks] == [0.0, 0.1]


def test_reference_quirks_are_kept():
    """CCT hard-wires seq_pool and dropout_rate in its call of TransformerClassifier: passing them raises TypeError; the
    `stochastic_depth` keyword is swallowed by **kwargs, `stochastic_depth_rate` is the knob."""
    base = dict(img_size=16, embedding_dim=64, num_layers=2, num_heads=2)
    for kw in (dict(seq_pool=False), dict(dropout_rate=0.1), dict(stochastic_depth=0.7)):
        with pytest.raises(TypeError):
            V.CCT(**base, **kw)
    c = V.TransformerClassifier(embedding_dim=64, num_layers=2, num_heads=2, sequence_length=4, stochastic_depth=0.7)
    assert [round(b.drop_path.drop_prob, 6) for b in c.blocks] == [0.0, 0.1]          # swallowed: the rate stays at its default
    m = V.CCT(**base, stochastic_depth_rate=0.4, an_unknown_keyword=1)
    assert [round(b.drop_path.drop_prob, 6) for b in m.classifier.blocks] == [0.0, 0.4]
    c = V.TransformerClassifier(True, 64, 2, 2, 2.0, 10, 0.0, 0.1, 0.1, "sine", 16, "extra positional", another=2)
    assert c.sequence_length == 16 and tuple(c.positional_emb.shape) == (1, 16, 64) and not c.positional_emb.requires_grad
    with pytest.raises(AssertionError):
        V.TransformerClassifier(embedding_dim=64, num_heads=2, positional_embedding="sine")       # no sequence length
    with pytest.raises(AssertionError):
        V.TransformerClassifier(embedding_dim=64, num_heads=2, positional_embedding="rotary", sequence_length=4)


def test_sine_table_is_bit_equal(fx):
    assert np.array_equal(V.sinusoidal_embedding(16, 64).numpy().view(np.int32), fx["sine.16x64"].view(np.int32))


def test_sequence_length_is_arithmetic():
    t = V.Tokenizer(7, 2, 3, n_conv_layers=2, n_output_channels=64, activation=torch.nn.ReLU)
    assert t.sequence_length(3, 30, 30) == 4 and t.plane(30, 30) == (2, 2)
    assert V.Tokenizer(7, 2, 3, n_output_channels=64).sequence_length() == 56 * 56
    assert V.Tokenizer(3, 1, 1, n_output_channels=64).sequence_length(3, 16, 24) == 8 * 12
    assert V.Tokenizer(3, 1, 1, 2, 2, 0, n_output_channels=64).sequence_length(3, 17, 17) == 64


@pytest.mark.parametrize("case", list(CF.CASES))
def test_module_tree_and_keys(fx, case):
    m = CF.build(V, case)
    PC.check_tree_and_keys(m, CF.weights(m, 3), fx, case)


def test_key_names():
    keys = set(CF.build(V, "k7x2").state_dict())
    assert {"tokenizer.conv_layers.0.0.weight", "tokenizer.conv_layers.1.0.weight", "classifier.positional_emb",
            "classifier.attention_pool.weight", "classifier.attention_pool.bias", "classifier.blocks.0.pre_norm.weight",
            "classifier.blocks.0.self_attn.qkv.weight", "classifier.blocks.0.self_attn.proj.bias", "classifier.blocks.1.linear1.weight",
            "classifier.blocks.1.norm1.bias", "classifier.blocks.1.linear2.bias", "classifier.norm.weight", "classifier.fc.bias"} <= keys
    assert "classifier.blocks.0.self_attn.qkv.bias" not in keys and "tokenizer.conv_layers.0.0.bias" not in keys
    assert "classifier.positional_emb" not in set(CF.build(V, "nopos").state_dict())
    cls = set(CF.build(V, "cls").state_dict())
    assert "class_emb" in cls and "attention_pool.weight" not in cls and tuple(CF.build(V, "cls").positional_emb.shape) == (1, 13, 64)


def test_seeded_init_matches_reference(fx):
    torch.manual_seed(0)
    PC.check_seeded_init(getattr(V, CF.FULL_BUILDER)(**CF.FULL), fx, "full")


@pytest.mark.parametrize("case", list(CF.CASES))
def test_restatement_reproduces_the_reference(fx, case):
    m = CF.build(V, case)
    m.load_state_dict(CF.weights(m, 3), strict=True)
    x, y = CF.inputs(case)
    masks = CF.unpack_masks(fx, case, len(CF.classifier_of(m).blocks)) if case == "drop" else None
    if masks is not None:
        keep = masks["path"][1]
        assert set(masks["path"]) == {1} and keep.shape == (2, 4) and bool((keep == 0).any()) and bool((keep == 1).any())
        assert 0.85 < float(masks["attn"][0].float().mean()) < 0.95
    result = R.cct_loss_and_grads(m, x, y, masks=masks)

    def noise(k, g):
        # attention_pool.bias: softmax is blind to a shift of its logits, the gradient is zero in exact arithmetic and
        # rounding noise (~1e-8) on both sides; a relative error of noise says nothing, so both must vanish
        if float(g.abs().max()) >= 1e-6:
            return False
        assert k.endswith("attention_pool.bias"), k
        return True
    PC.check_restatement(result, fx, case, m.training, noise=noise)
    if m.training:
        assert {k for k, g in result[2].items() if g is None} <= {"classifier.positional_emb"}       # the frozen sine table


def test_refused_configurations():
    base = dict(img_size=16, embedding_dim=64, num_layers=1, num_heads=2, mlp_ratio=2, num_classes=10)
    for kw in (dict(embedding_dim=60), dict(embedding_dim=4104, num_heads=1), dict(mlp_ratio=0.3), dict(num_heads=4),
               dict(kernel_size=9, padding=4), dict(pooling_kernel_size=4), dict(pooling_stride=4), dict(pooling_padding=2),
               dict(img_size=640, kernel_size=3, stride=1, padding=1, pooling_stride=1)):
        with pytest.raises(NotImplementedError):
            V.CCT(**dict(base, **kw))                                   # num_heads=4: head dim 16; the last: 409600 tokens
    for kw in (dict(activation=torch.nn.GELU), dict(max_pool=False), dict(conv_bias=True), dict(n_conv_layers=2, in_planes=60),
               dict(n_output_channels=60)):
        with pytest.raises(NotImplementedError):
            V.Tokenizer(3, 1, 1, **kw)
    assert V.Tokenizer(3, 1, 1, activation=None)._geom[0][3] is False      # legal in the reference: pool without ReLU
    img = torch.zeros(1, 3, 16, 16)
    with pytest.raises(NotImplementedError):
        V.CCT(**base)(PC.fake_cuda(torch.zeros(1, 3, 16, 24)))               # not the constructed size
    with pytest.raises(NotImplementedError):
        V.TransformerClassifier(embedding_dim=64, num_heads=2, num_layers=1, dropout_rate=0.1, sequence_length=4).train()(
            PC.fake_cuda(torch.zeros(1, 4, 64)))
    with pytest.raises(NotImplementedError):
        V.TransformerClassifier(embedding_dim=64, num_heads=2, num_layers=1, dropout_rate=0.0, sequence_length=4)(
            PC.fake_cuda(torch.zeros(1, 3, 64)))                             # fewer tokens: the reference's padding branch is broken
    with pytest.raises(NotImplementedError):
        V.TransformerClassifier(embedding_dim=64, num_heads=2, num_layers=1, positional_embedding="none")(
            PC.fake_cuda(torch.zeros(1, 5000, 64)))
    with pytest.raises(NotImplementedError):
        V.TransformerEncoderLayer(64, 2, 128, dropout=0.1).train()(PC.fake_cuda(torch.zeros(1, 4, 64)))
    from noise_robust_vit_amd.encoder import record_attention
    with record_attention([]):
        with pytest.raises(NotImplementedError):
            V.CCT(**base)(PC.fake_cuda(img))
    with pytest.raises(NotImplementedError):
        V.Attention(64, 2)(torch.zeros(1, 4, 64))                          # a holder: the block runs as a whole
    from noise_robust_vit_amd._lib import NrvError
    m = V.CCT(**base)
    for call in (lambda: m(img), lambda: m.tokenizer(img), lambda: m.classifier(torch.zeros(1, 64, 64)),
                 lambda: m.classifier.blocks[0](torch.zeros(1, 64, 64)), lambda: V.DropPath(0.5).train()(torch.zeros(2, 4))):
        with pytest.raises(NrvError):
            call()                                                          # CPU tensors: no fallback


def test_new_prototypes_are_declared_bound_and_exported():
    PC.check_prototypes(NEW, source="nrv_cct.hip", wrappers=("relu_maxpool_fwd", "relu_maxpool_bwd", "layernorm_f32_fwd",
                                                              "layernorm_f32_bwd", "seqpool_fwd", "seqpool_bwd"))


def test_pool_entry_points_answer_without_a_device(lib):
    """Shapes first (NRV_ERR_SHAPE), then pointers, the dtype and the alignment; every call returns before a launch."""
    z, ok, odd = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    good = (2, 5, 7, 64, 3, 2, 1)                                          # B, H, W, C, pk, ps, pp
    assert lib.nrv_relu_maxpool_fwd(z, 0, 1, z, z, z, *good, None) == ERR_NULL
    assert lib.nrv_relu_maxpool_bwd(z, z, z, *good, None) == ERR_NULL
    for bad in ((2, 5, 7, 60, 3, 2, 1), (2, 5, 7, 64, 4, 2, 1), (2, 5, 7, 64, 1, 1, 0), (2, 5, 7, 64, 3, 4, 1), (2, 5, 7, 64, 3, 0, 1),
                (2, 5, 7, 64, 3, 2, 2), (2, 5, 7, 64, 2, 2, 2), (2, 5, 7, 64, 3, 2, -1), (0, 5, 7, 64, 3, 2, 1), (2, 0, 7, 64, 3, 2, 1),
                (2, 1, 1, 64, 2, 2, 0), (2, 5000, 5000, 64, 3, 2, 1)):
        assert lib.nrv_relu_maxpool_fwd(z, 0, 1, z, z, z, *bad, None) == ERR_SHAPE, bad
        assert lib.nrv_relu_maxpool_bwd(z, z, z, *bad, None) == ERR_SHAPE, bad
    assert lib.nrv_relu_maxpool_fwd(z, 0, 1, z, z, z, 2, 1, 1, 8, 3, 1, 1, None) == ERR_NULL    # a 1 x 1 plane under (3, 1, 1) is a shape
    assert lib.nrv_relu_maxpool_fwd(ok, 0, 1, z, z, ok, *good, None) == ERR_NULL                # neither output
    assert lib.nrv_relu_maxpool_fwd(ok, 0, 1, ok, z, z, *good, None) == ERR_NULL                # no idx
    assert lib.nrv_relu_maxpool_fwd(ok, 7, 1, ok, z, ok, *good, None) == ERR_DTYPE
    for k in (0, 3, 4, 5):
        a = [ok, 1, 1, ok, ok, ok]
        a[k] = odd
        assert lib.nrv_relu_maxpool_fwd(*a, *good, None) == ERR_ALIGN, k
    for k in range(3):
        a = [ok] * 3
        a[k] = z
        assert lib.nrv_relu_maxpool_bwd(*a, *good, None) == ERR_NULL, k
        a[k] = odd
        assert lib.nrv_relu_maxpool_bwd(*a, *good, None) == ERR_ALIGN, k


def test_layernorm_f32_entry_points_answer_without_a_device(lib):
    z, ok, odd = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    eps = ctypes.c_float(1e-5)
    assert lib.nrv_layernorm_f32_fwd(z, z, z, z, z, z, z, 5, 64, eps, None) == ERR_NULL
    for rows, dim in ((5, 60), (5, 4), (5, 4104), (0, 64), (5, 0)):
        assert lib.nrv_layernorm_f32_fwd(z, z, z, z, z, z, z, rows, dim, eps, None) == ERR_SHAPE, (rows, dim)
        assert lib.nrv_layernorm_f32_bwd(z, z, z, z, z, z, z, z, z, z, 0, rows, dim, None) == ERR_SHAPE, (rows, dim)
        assert lib.nrv_layernorm_f32_bwd_workspace(rows, dim) == 0
    assert lib.nrv_layernorm_f32_fwd(z, z, z, z, z, z, z, 1, 4096, eps, None) == ERR_NULL     # the widest row, one row: a shape
    for k in (0, 1, 2, 3, 5, 6):
        a = [ok] * 7
        a[k] = z
        assert lib.nrv_layernorm_f32_fwd(*a, 5, 64, eps, None) == ERR_NULL, k
    for k in (0, 1, 2, 3, 4):
        a = [ok] * 7
        a[k] = odd
        assert lib.nrv_layernorm_f32_fwd(*a, 5, 64, eps, None) == ERR_ALIGN, k
    need = lib.nrv_layernorm_f32_bwd_workspace(37, 64)
    assert need == 2 * 2 * 64 * 4                                           # five waves of 8 rows in two workgroups: a dgamma and a dbeta row each
    assert lib.nrv_layernorm_f32_bwd_workspace(50432, 768) == 970 * 2 * 768 * 4        # 13 rows per wave, 3880 waves, 970 workgroups
    for k in (0, 1, 2, 3, 4, 5, 7, 8, 9):
        a = [ok] * 10
        a[k] = z
        assert lib.nrv_layernorm_f32_bwd(*a, need, 37, 64, None) == ERR_NULL, k
    assert lib.nrv_layernorm_f32_bwd(*[ok] * 10, need - 1, 37, 64, None) == ERR_WORKSPACE
    for k in (0, 1, 2, 5, 6, 9):
        a = [ok] * 10
        a[k] = odd
        assert lib.nrv_layernorm_f32_bwd(*a, need, 37, 64, None) == ERR_ALIGN, k


def test_seqpool_entry_points_answer_without_a_device(lib):
    z, ok, odd = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    assert lib.nrv_seqpool_fwd(z, z, z, z, z, 3, 4096, 4096, None) == ERR_NULL         # the largest shape is a shape
    assert lib.nrv_seqpool_fwd(z, z, z, z, z, 3, 1, 8, None) == ERR_NULL
    for B, n, D in ((3, 4097, 64), (3, 0, 64), (0, 16, 64), (3, 16, 60), (3, 16, 4), (3, 16, 4104)):
        assert lib.nrv_seqpool_fwd(z, z, z, z, z, B, n, D, None) == ERR_SHAPE, (B, n, D)
        assert lib.nrv_seqpool_bwd(z, z, z, z, z, z, z, z, 0, B, n, D, None) == ERR_SHAPE, (B, n, D)
    for k in range(5):
        a = [ok] * 5
        a[k] = z
        assert lib.nrv_seqpool_fwd(*a, 3, 16, 64, None) == ERR_NULL, k
    for k in (0, 1):
        a = [ok] * 5
        a[k] = odd
        assert lib.nrv_seqpool_fwd(*a, 3, 16, 64, None) == ERR_ALIGN, k
    need = lib.nrv_seqpool_bwd_workspace(3, 64)
    assert need == (3 * 64 + 3) * 4 and lib.nrv_seqpool_bwd_workspace(3, 60) == 0
    for k in range(8):
        a = [ok] * 8
        a[k] = z
        assert lib.nrv_seqpool_bwd(*a, need, 3, 16, 64, None) == ERR_NULL, k
    assert lib.nrv_seqpool_bwd(*[ok] * 8, need - 1, 3, 16, 64, None) == ERR_WORKSPACE
    for k in (0, 1):
        a = [ok] * 8
        a[k] = odd
        assert lib.nrv_seqpool_bwd(*a, need, 3, 16, 64, None) == ERR_ALIGN, k


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from noise_robust_vit_amd import kernels as K
    from noise_robust_vit_amd._lib import NrvError
    for call in (lambda: K.relu_maxpool_fwd(torch.zeros(18, 8), 2, 3, 3, 3, 2, 1),
                 lambda: K.relu_maxpool_bwd(torch.zeros(8, 8), torch.zeros(8, 8, dtype=torch.uint8), 2, 3, 3, 3, 2, 1),
                 lambda: K.layernorm_f32_fwd(torch.zeros(4, 8), torch.ones(8), torch.zeros(8), 1e-5),
                 lambda: K.layernorm_f32_bwd(torch.zeros(4, 8), torch.zeros(4, 8), torch.ones(8), torch.zeros(4), torch.ones(4)),
                 lambda: K.seqpool_fwd(torch.zeros(8, 8), torch.zeros(8), torch.zeros(1), 2, 4),
                 lambda: K.seqpool_bwd(torch.zeros(2, 8), torch.zeros(8, 8), torch.zeros(8), torch.zeros(2, 4), 2, 4),
                 lambda: K.relu_maxpool_fwd(PC.fake_cuda(torch.zeros(18, 8)), 2, 3, 3, 4, 2, 1),            # pooling kernel 4
                 lambda: K.relu_maxpool_fwd(PC.fake_cuda(torch.zeros(18, 12)), 2, 3, 3, 3, 2, 1),           # C % 8
                 lambda: K.layernorm_f32_fwd(PC.fake_cuda(torch.zeros(4, 12)), torch.ones(12), torch.zeros(12), 1e-5),
                 lambda: K.seqpool_fwd(PC.fake_cuda(torch.zeros(8, 8)), PC.fake_cuda(torch.zeros(8)), PC.fake_cuda(torch.zeros(1)), 2, 5)):
        with pytest.raises(NrvError):
            call()
