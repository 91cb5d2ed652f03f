"""Reference chain of the joint-embedding baseline (model/embedding_net.py:130-162, 220-314; model/multimodal_context_net.py:9-61; model/tcn.py;
train_eval/train_joint_embed.py:5-51) restated with stock torch.nn modules under the reference's state_dict keys.  Unlike the reference's own
modules it takes injected draws (eps of reparameterize, dropout masks), so that it can be compared with the HIP path draw for draw, and runs in
fp64 (the tests' reference) or fp32 (the benchmark's comparator).  make_state(seed, n_words) is the seeded state maker: fixtures and tests
hold seeds and inputs, never the 7 M-parameter state."""
import random
import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import _VF


# Linear / Conv biases directly followed by a train-mode BatchNorm: the normalisation removes the column mean, so their gradient is EXACTLY zero
# and both sides hold only rounding noise there.  max|delta| / max|ref| is undefined for them; the tests measure these tensors against the
# largest magnitude of the sibling weight gradient (the bias gradient is a column sum of the dy that forms it), and leave them out of the
# stepped-parameter comparison (Adam turns the noise's sign into steps of lr).  An explicit list: any other tensor with a wrongly zero
# gradient fails its plain comparison.
ZERO_GRAD_BIASES = tuple(f"context_encoder.audio_encoder.feat_extractor.{i}.bias" for i in (0, 3, 6)) + ("context_encoder.out.0.bias",) + \
    tuple(f"pose_encoder.net.{i}.0.bias" for i in (0, 1, 2)) + ("pose_encoder.net.3.bias", "pose_encoder.out_net.0.bias", "pose_encoder.out_net.1.bias",
                                                               "pose_encoder.out_net.3.bias", "decoder.pre_pose_net.0.bias")
# (pose_encoder.net.3.bias: the last conv's bias is a per-channel constant, the flatten and Linear(384, 256) that follow are linear, so it
# reaches the train-mode BatchNorm behind them as a per-column constant too.  pose_encoder.out_net.1.bias: the first BatchNorm's beta passes
# LeakyReLU(True) -- the identity -- and Linear(256, 128) into the second BatchNorm.  Every other bias or beta meets a real non-linearity, the
# GRU, or a BatchNorm over positions where it is not constant, before any batch normalisation.)

_PROBE = None          # relu_stats(): name -> input of every functional ReLU of the chain


def _relu(x, name):
    if _PROBE is not None:
        _PROBE[name] = x.detach()
    return F.relu(x)


class _Chomp(nn.Module):
    def __init__(self, n):
        super().__init__(); self.n = n

    def forward(self, x):
        return x[:, :, :-self.n].contiguous()


def _wn(cin, cout, d):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return torch.nn.utils.weight_norm(nn.Conv1d(cin, cout, 2, stride=1, padding=d, dilation=d))


class _Block(nn.Module):                                       # model/tcn.py:17-47
    def __init__(self, c, d, p):
        super().__init__()
        self.conv1, self.conv2 = _wn(c, c, d), _wn(c, c, d)
        self.net = nn.Sequential(self.conv1, _Chomp(d), nn.ReLU(), nn.Dropout(p), self.conv2, _Chomp(d), nn.ReLU(), nn.Dropout(p))
        self.d = d

    def forward(self, x, m1=None, m2=None):                    # masks (B, T, C) or None (no dropout)
        o = _relu(self.conv1(x)[:, :, :-self.d], f"tcn.d{self.d}.conv1")
        o = o if m1 is None else o * m1.transpose(1, 2)
        o = _relu(self.conv2(o)[:, :, :-self.d], f"tcn.d{self.d}.conv2")
        o = o if m2 is None else o * m2.transpose(1, 2)
        return _relu(o + x, f"tcn.d{self.d}.residual")


class _TCN(nn.Module):
    def __init__(self, c, n, p):
        super().__init__()
        self.network = nn.Sequential(*[_Block(c, 2 ** i, p) for i in range(n)])


class TextEncoder(nn.Module):                                  # multimodal_context_net.py:31-61
    def __init__(self, n_words, embed, hidden, n_layers):
        super().__init__()
        self.embedding = nn.Embedding(n_words, embed)
        self.tcn = _TCN(hidden, n_layers, 0.3)
        self.decoder = nn.Linear(hidden, 32)

    def forward(self, ids, draws):
        e = self.embedding(ids)
        if "c.emb_drop" in draws:
            e = e * draws["c.emb_drop"]
        x = e.transpose(1, 2)
        for i, blk in enumerate(self.tcn.network):
            x = blk(x, draws.get(f"c.tcn{i}.drop1"), draws.get(f"c.tcn{i}.drop2"))
        return self.decoder(x.transpose(1, 2))


class WavEncoder(nn.Module):                                   # multimodal_context_net.py:9-28
    def __init__(self):
        super().__init__()
        self.feat_extractor = nn.Sequential(
            nn.Conv1d(1, 16, 15, stride=5, padding=1600), nn.BatchNorm1d(16), nn.LeakyReLU(0.3, inplace=True),
            nn.Conv1d(16, 32, 15, stride=6), nn.BatchNorm1d(32), nn.LeakyReLU(0.3, inplace=True),
            nn.Conv1d(32, 64, 15, stride=6), nn.BatchNorm1d(64), nn.LeakyReLU(0.3, inplace=True),
            nn.Conv1d(64, 32, 15, stride=6))

    def forward(self, wav):
        return self.feat_extractor(wav.unsqueeze(1)).transpose(1, 2)


def gru_stack(x, gru, masks=None):
    """nn.GRU's arithmetic layer by layer (batch_first), with the inter-layer dropout as injected scale masks {layer: (B, T, D H)}."""
    D = 2 if gru.bidirectional else 1
    for l in range(gru.num_layers):
        ws = [getattr(gru, f"{n}_l{l}{s}") for s in (("", "_reverse") if D == 2 else ("",)) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        h0 = x.new_zeros(D, x.shape[0], gru.hidden_size)
        x = _VF.gru(x, h0, ws, True, 1, 0.0, torch.is_grad_enabled(), D == 2, True)[0]       # (train flag: MIOpen's backward wants it; dropout is 0)
        if masks is not None and l < gru.num_layers - 1 and l in masks:
            x = x * masks[l]
    return x


class ContextEncoder(nn.Module):                               # embedding_net.py:220-259
    def __init__(self, n_words, embed, hidden, n_layers):
        super().__init__()
        self.text_encoder = TextEncoder(n_words, embed, hidden, n_layers)
        self.audio_encoder = WavEncoder()
        self.gru = nn.GRU(64, hidden_size=256, num_layers=2, bidirectional=False, batch_first=True)
        self.out = nn.Sequential(nn.Linear(256, 128), nn.BatchNorm1d(128), nn.ReLU(inplace=True), nn.Linear(128, 32))
        self.fc_mu, self.fc_logvar = nn.Linear(32, 32), nn.Linear(32, 32)

    def forward(self, ids, wav, draws):
        x = torch.cat((self.audio_encoder(wav), self.text_encoder(ids, draws)), dim=2)
        out = self.out(gru_stack(x, self.gru)[:, -1])
        mu, logvar = self.fc_mu(out), self.fc_logvar(out)
        return mu + draws["c.eps"] * torch.exp(0.5 * logvar), mu, logvar


def _cnr(cin, cout, down=False):
    k, s = (4, 2) if down else (3, 1)
    return nn.Sequential(nn.Conv1d(cin, cout, k, stride=s), nn.BatchNorm1d(cout), nn.LeakyReLU(0.2, True))


class PoseEncoderConv(nn.Module):                              # embedding_net.py:42-82
    def __init__(self, dim):
        super().__init__()
        self.net = nn.Sequential(_cnr(dim, 32), _cnr(32, 64), _cnr(64, 64, True), nn.Conv1d(64, 32, 3))
        self.out_net = nn.Sequential(nn.Linear(384, 256), nn.BatchNorm1d(256), nn.LeakyReLU(True), nn.Linear(256, 128), nn.BatchNorm1d(128),
                                     nn.LeakyReLU(True), nn.Linear(128, 32))
        self.fc_mu, self.fc_logvar = nn.Linear(32, 32), nn.Linear(32, 32)

    def forward(self, poses):
        out = self.out_net(self.net(poses.transpose(1, 2)).flatten(1))
        mu = self.fc_mu(out)
        return mu, mu, self.fc_logvar(out)


class PoseDecoderGRU(nn.Module):                               # embedding_net.py:130-162
    def __init__(self, gen_length, pose_dim):
        super().__init__()
        self.gen_length = gen_length
        self.pre_pose_net = nn.Sequential(nn.Linear(pose_dim * 4, 32), nn.BatchNorm1d(32), nn.ReLU(), nn.Linear(32, 32))
        self.gru = nn.GRU(64, hidden_size=300, num_layers=4, batch_first=True, bidirectional=True, dropout=0.3)
        self.out = nn.Sequential(nn.Linear(300, 150), nn.LeakyReLU(True), nn.Linear(150, pose_dim))

    def forward(self, latent, pre_poses, draws):
        feat = torch.cat((self.pre_pose_net(pre_poses.reshape(pre_poses.shape[0], -1)), latent), dim=1)
        masks = {l: draws[f"g.gru.drop{l}"] for l in range(3) if f"g.gru.drop{l}" in draws}
        y = gru_stack(feat.unsqueeze(1).repeat(1, self.gen_length, 1), self.gru, masks)
        y = y[:, :, :300] + y[:, :, 300:]
        return self.out(y.reshape(-1, 300)).view(pre_poses.shape[0], self.gen_length, -1)


class EmbeddingNet(nn.Module):                                 # embedding_net.py:262-308 (mode != 'pose')
    def __init__(self, pose_dim=27, n_frames=34, n_words=32, embed=300, hidden=300, n_layers=4, mode="random"):
        super().__init__()
        self.context_encoder = ContextEncoder(n_words, embed, hidden, n_layers)
        self.pose_encoder = PoseEncoderConv(pose_dim)
        self.decoder = PoseDecoderGRU(n_frames, pose_dim)
        self.mode = mode

    def forward(self, in_text, in_audio, pre_poses, poses, input_mode=None, draws=None):
        draws = draws or {}
        input_mode = self.mode if input_mode is None else input_mode
        c = (None, None, None) if in_text is None or in_audio is None else self.context_encoder(in_text, in_audio, draws)
        p = (None, None, None) if poses is None else self.pose_encoder(poses)
        if input_mode == "random":
            input_mode = "speech" if random.random() > 0.5 else "pose"
        latent = c[0] if input_mode == "speech" else p[0]
        return c + p + (self.decoder(latent, pre_poses, draws),)


def make_state(seed, n_words=32, embed=300, hidden=300, n_layers=4):
    """Seeded fp32 state dict under the reference's keys: torch's default initialisation, with the BatchNorm affine parameters and running
    statistics moved off their trivial initial values so that every term of the normalisation is exercised."""
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    net = EmbeddingNet(n_words=n_words, embed=embed, hidden=hidden, n_layers=n_layers)
    sd = net.state_dict()
    for k, v in sd.items():
        if k.endswith("running_mean"):
            v.copy_(0.1 * torch.randn(v.shape, generator=g))
        elif k.endswith("running_var"):
            v.copy_(0.5 + torch.rand(v.shape, generator=g))
        elif k.endswith("num_batches_tracked"):
            v.fill_(3)
        elif "weight_v" in k:
            v.copy_(0.05 * torch.randn(v.shape, generator=g))
        elif k.endswith("embedding.weight"):
            v.copy_(0.5 * torch.randn(v.shape, generator=g))
    for name, m in net.named_modules():
        if isinstance(m, nn.BatchNorm1d):
            sd[name + ".weight"].copy_(0.5 + torch.rand(m.num_features, generator=g))
            sd[name + ".bias"].copy_(0.1 * torch.randn(m.num_features, generator=g))
    return {k: v.clone() for k, v in sd.items()}


def make_inputs(seed, B, n_words=32, samples=36267, pose_dim=27, n_frames=34, drop_p=0.0):
    """Seeded inputs and draws: word ids, audio, target poses, eps; with drop_p > 0 the decoder GRU's inverted-dropout masks."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, n_words, (B, n_frames), generator=g)
    audio = 0.1 * torch.randn(B, samples, generator=g)
    target = 0.5 * torch.randn(B, n_frames, pose_dim, generator=g)
    draws = {"c.eps": torch.randn(B, 32, generator=g)}
    if drop_p > 0:
        for l in range(3):
            draws[f"g.gru.drop{l}"] = (torch.rand(B, n_frames, 600, generator=g) >= drop_p).float() / (1 - drop_p)
    return ids, audio, target, draws


def build(state, dtype=torch.float64, device="cpu", mode="random"):
    n_words, embed = state["context_encoder.text_encoder.embedding.weight"].shape
    net = EmbeddingNet(n_words=n_words, embed=embed, mode=mode)
    net.load_state_dict(state, strict=True)
    return net.to(device=device, dtype=dtype)


def embed_loss(recon, target):
    """train_joint_embed.py:20-28: sum over clips of the clip's mean L1."""
    return F.l1_loss(recon, target, reduction="none").mean(dim=(1, 2)).sum()


def train_iter_embed(net, optim, in_text, in_audio, target, mode, draws, n_pre=4):
    """train_joint_embed.py:5-51 (variational_encoding False on both branches: no KLD)."""
    optim.zero_grad()
    out = net(in_text, in_audio, target[:, :n_pre], target, mode, draws)
    loss = embed_loss(out[6], target)
    loss.backward()
    optim.step()
    return float(loss)


def relu_stats(net, in_text, in_audio, target, mode, draws, n_pre=4, rel=1e-4):
    """Near-tie census of one forward: for the input x of every ReLU / LeakyReLU (module or functional; LeakyReLU(True) has slope 1 and is the
    identity: skipped) -> {name: {'numel', 'near', 'margin'}}: `near` counts the elements with 0 < |x| < rel max|x|, `margin` is the
    smallest non-zero |x| / max|x|.  Exact zeros are skipped (both sides of the kink give 0 there), and so is a tensor without negative
    elements (the ReLU after the sum of two post-ReLU tensors in the TCN's later blocks: the identity)."""
    global _PROBE
    seen, hooks = {}, []
    for name, m in net.named_modules():
        if isinstance(m, nn.ReLU) or (isinstance(m, nn.LeakyReLU) and m.negative_slope != 1):
            hooks.append(m.register_forward_pre_hook(lambda _m, inp, name=name: seen.__setitem__(name, inp[0].detach().clone())))
    _PROBE = seen
    try:
        with torch.no_grad():
            net(in_text, in_audio, target[:, :n_pre], target, mode, draws)
    finally:
        _PROBE = None
        for h in hooks:
            h.remove()
    out = {}
    for name, x in seen.items():
        if float(x.min()) >= 0:
            continue
        ax = x.abs()
        nz = ax[ax > 0]
        out[name] = {"numel": x.numel(), "near": int((nz < rel * ax.max()).sum()), "margin": float(nz.min() / ax.max())}
    return out
