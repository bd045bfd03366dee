"""HipImageEncoder(dtype="float32") without a GPU: the orchestration of HipImageEncoder._forward_f32 runs on the torch-CPU restatements of
its four kernels (tests/_f32_backend.TorchBackend) against oracle.dinov2_oracle.dinov2_forward, and its launches are counted.  The same
assertions run on the kernels in tests/test_fp32_path_gpu.py.

Two tiny models cover both head dims am_attention_f32 has: 2 layers, 2 heads, T = 2 frames; hidden_size 128 (head_dim 64) on 28 x 42
pixels and hidden_size 256 (head_dim 128) on 42 x 28 - non-square images, so the 37 x 37 position table is resampled.
Bound: rel-L2 <= 2e-5, the bound every fp32 model test here uses (tests/_stage1_fp32.py).  A plain-torch restatement of this packing
(stacked q | k | v, LayerScale folded into the out-projection and fc2) sits at 4.4e-7 and 3.9e-7 on the two cases."""
import pytest
import torch

from _f32_backend import TorchBackend

BOUND = 2e-5
T, NL = 2, 2
CASES = {"head_dim_64": (128, 28, 42), "head_dim_128": (256, 42, 28)}           # hidden_size, height, width
CPU = torch.device("cpu")


def check_case(name, dev, backend=None):
    """The fp32 encoder on `dev` (with `backend` in place of the HIP kernels when given) against the oracle; its launches counted."""
    from actionmesh_amd import HipImageEncoder
    from oracle import dinov2_oracle as DO
    C, height, width = CASES[name]
    cfg = DO.DinoConfig(hidden_size=C, num_hidden_layers=NL, num_attention_heads=2)
    sd = DO.synthetic_state_dict(cfg, seed=3)
    pixels = torch.randn((T, 3, height, width), generator=torch.Generator().manual_seed(C + height))
    ref = DO.dinov2_forward(sd, cfg, pixels)
    enc = HipImageEncoder(config=vars(cfg), state_dict=sd, dtype="float32")
    enc.f32_backend = backend
    enc.to(dev)
    assert enc.entry_counts() == ({} if backend is None else backend.calls) == {}
    out = enc.encode_pixels(pixels.to(dev)).cpu()
    assert out.shape == ref.shape == (T, 1 + (height // 14) * (width // 14), C) and out.dtype == torch.float32
    r = float((out.double() - ref.double()).norm() / ref.double().norm())
    print(f"fp32 encoder {name}: rel-L2 vs the oracle {r:.3e}")
    assert r <= BOUND, (name, r)
    assert enc.entry_counts() == {"am_patchify_f32": 1, "am_gemm_f32": T + 4 * NL, "am_layernorm_f32": 2 * NL + 1, "am_attention_f32": NL}
    return enc


@pytest.mark.parametrize("name", list(CASES))
def test_encoder_fp32_against_the_oracle(name):
    backend = TorchBackend()
    enc = check_case(name, CPU, backend)
    assert enc.entry_counts() == backend.calls


def test_a_16_bit_encoder_counts_nothing_and_fp32_without_a_backend_needs_the_device():
    from actionmesh_amd import HipImageEncoder
    from oracle import dinov2_oracle as DO
    cfg = DO.DinoConfig(hidden_size=128, num_hidden_layers=NL, num_attention_heads=2)
    sd = DO.synthetic_state_dict(cfg, seed=3)
    assert HipImageEncoder(config=vars(cfg), state_dict=sd).entry_counts() == {}
    enc = HipImageEncoder(config=vars(cfg), state_dict=sd, dtype="float32")
    with pytest.raises(RuntimeError, match="no CPU path"):
        enc.encode_pixels(torch.zeros((T, 3, 28, 42)))
    enc16 = HipImageEncoder(config=vars(cfg), state_dict=sd)
    enc16.f32_backend = TorchBackend()                                   # a backend does not take a 16-bit model off the device
    with pytest.raises(RuntimeError, match="no CPU path"):
        enc16.encode_pixels(torch.zeros((T, 3, 28, 42)))
