"""Seeded parameters and inputs of the Speech2Gesture tests, shared by tests/golden/make_golden_s2g.py (on the reference's modules) and the
GPU tests (on this package's): the full generator is 26 MB, so it is regenerated from the seed instead of stored."""
import torch


def fill_state(module, seed):
    """Deterministic values for every parameter, in state_dict order: conv / linear weights U(-1/sqrt(fan_in), +), biases 0.1 N(0, 1),
    BatchNorm gamma 1 + 0.1 N, beta 0.1 N; running statistics keep their defaults."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name.endswith("weight") and p.dim() >= 2:
                bound = 1.0 / (p[0].numel() ** 0.5)
                p.copy_((torch.rand(p.shape, generator=g, dtype=torch.float64) * 2 - 1) * bound)
            elif name.endswith("weight"):
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g, dtype=torch.float64))
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=g, dtype=torch.float64))
    return module


def make_inputs(B, seed, n_mels=128, frames=70, n_poses=34, pose_dim=27):
    """(in_spec fp16 (B, n_mels, frames) like the loader's log-mel spectrogram, target poses fp32 (B, n_poses, pose_dim))."""
    g = torch.Generator().manual_seed(seed)
    spec = (torch.randn(B, n_mels, frames, generator=g) * 2 - 3).to(torch.float16)
    poses = torch.cumsum(0.1 * torch.randn(B, n_poses, pose_dim, generator=g), dim=1)
    return spec, poses
