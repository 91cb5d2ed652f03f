"""tests/joint_embed_ref.py extended by the variational switch (embedding_net.py:77-80, train_joint_embed.py:30-50 with
variational_encoding=True): the same fp64 modules, the pose encoder reparameterised with the injected draw 'p.eps'."""
import random

import torch

import joint_embed_ref as R
import vae_ref as VR


def forward_variational(net, in_text, in_audio, pre_poses, poses, input_mode, draws):
    """R.EmbeddingNet.forward with variational_encoding=True -> the reference's 7-tuple."""
    input_mode = net.mode if input_mode is None else input_mode
    c = (None, None, None) if in_text is None or in_audio is None else net.context_encoder(in_text, in_audio, draws)
    enc = net.pose_encoder
    out = enc.out_net(enc.net(poses.transpose(1, 2)).flatten(1))
    mu, logvar = enc.fc_mu(out), enc.fc_logvar(out)
    p = (mu + draws["p.eps"] * torch.exp(0.5 * logvar), mu, logvar)
    if input_mode == "random":
        input_mode = "speech" if random.random() > 0.5 else "pose"
    latent = c[0] if input_mode == "speech" else p[0]
    return c + p + (net.decoder(latent, pre_poses, draws),)


def train_iter_embed_variational(net, epoch, in_text, in_audio, target, mode, draws, loss_regression_weight, loss_kld_weight, n_pre=4):
    """-> ({'loss': recon, 'KLD': KLD}, gradients by name): backward only, no optimiser step."""
    net.zero_grad()
    out = forward_variational(net, in_text, in_audio, target[:, :n_pre], target, mode, draws)
    mu, logvar = (out[1], out[2]) if net.mode == "speech" else (out[4], out[5])
    loss, ret = VR.embed_vae_loss(out[6], target, mu, logvar, epoch, loss_regression_weight, loss_kld_weight)
    loss.backward()
    return ret, {k: (None if p.grad is None else p.grad.clone()) for k, p in net.named_parameters()}
