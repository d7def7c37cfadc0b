"""3D U-Net voxel encoder in plain PyTorch (counterpart of generators/unet3d.py:487-827 in the reference; it stays stock
PyTorch-ROCm per the north star).  Voxels (B,4,V,V,V) -> feature volume (B,out_channels,V,V,V) and, with
return_global=True, the spatial mean of the deepest level (B, f_maps * 2**(num_levels-1)) that drives the FiLM mapping.

Module names follow the reference (encoders.{i}.basic_module.SingleConv{1,2}.{groupnorm,conv}, decoders.{i}..., final_conv)
so `encoder_state_dict` of its checkpoints loads; 4,083,592 parameters at f_maps=32, num_levels=4.
Layer order 'gcr': GroupNorm (on the conv's input channels) -> Conv3d 3x3x3 without bias -> ReLU."""
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F


def _gcr(c_in, c_out, num_groups=8):
    groups = num_groups if c_in >= num_groups else 1
    return nn.Sequential(OrderedDict([("groupnorm", nn.GroupNorm(groups, c_in)),
                                      ("conv", nn.Conv3d(c_in, c_out, 3, padding=1, bias=False)),
                                      ("ReLU", nn.ReLU(inplace=True))]))


def _double_conv(c_in, c_out, encoder, num_groups=8):
    """Encoder side widens in two steps (c_in -> max(c_out/2, c_in) -> c_out), decoder side c_in -> c_out -> c_out."""
    mid = max(c_out // 2, c_in) if encoder else c_out
    return nn.Sequential(OrderedDict([("SingleConv1", _gcr(c_in, mid, num_groups)), ("SingleConv2", _gcr(mid, c_out, num_groups))]))


class _Down(nn.Module):
    def __init__(self, c_in, c_out, pool):
        super().__init__()
        self.pooling = nn.MaxPool3d(2) if pool else None
        self.basic_module = _double_conv(c_in, c_out, encoder=True)

    def forward(self, x):
        return self.basic_module(x if self.pooling is None else self.pooling(x))


class _Up(nn.Module):
    def __init__(self, c_in, c_out):
        super().__init__()
        self.basic_module = _double_conv(c_in, c_out, encoder=False)

    def forward(self, skip, x):
        x = F.interpolate(x, size=skip.shape[2:], mode="nearest")
        return self.basic_module(torch.cat((skip, x), dim=1))


class UNet3D(nn.Module):
    def __init__(self, in_channels=4, out_channels=32, f_maps=32, num_levels=4, return_global=True,
                 feature_volume_channels_last=True, **_ignored):
        super().__init__()
        self.feature_volume_channels_last = feature_volume_channels_last
        widths = [f_maps * 2 ** k for k in range(num_levels)] if isinstance(f_maps, int) else list(f_maps)
        self.encoders = nn.ModuleList(_Down(in_channels if i == 0 else widths[i - 1], w, pool=i > 0) for i, w in enumerate(widths))
        rev = widths[::-1]
        self.decoders = nn.ModuleList(_Up(rev[i] + rev[i + 1], rev[i + 1]) for i in range(len(rev) - 1))
        self.final_conv = nn.Conv3d(widths[0], out_channels, 1)
        self.return_global = return_global

    def forward(self, x):
        skips = []
        for enc in self.encoders:
            x = enc(x)
            skips.insert(0, x)
        glob = x.mean(dim=(2, 3, 4)) if self.return_global else None
        for dec, skip in zip(self.decoders, skips[1:]):
            x = dec(skip, x)
        x = self._final(x)
        return (x, glob) if self.return_global else x

    def _final(self, x):
        """The final 1x1x1 convolution (unet3d.py:593), written channel-last: a 1x1x1 convolution is the GEMM
        (B, V^3, f_maps) x (f_maps, out) -- evaluated in that orientation (rocBLAS reads the channel-first activations through
        a transposed operand, no copy) its output IS the (B,V,V,V,C) layout the render kernels gather from, one 128-byte line
        per trilinear corner.  The tensor handed on is the usual (B,C,V,V,V) view of it (torch.channels_last_3d strides), which
        ops.channel_last() takes as it is: the hand-off to the render path costs no transpose kernel and no copy, forward or
        backward.  Same parameters (`final_conv.weight/bias`), same values up to summation order."""
        if not self.feature_volume_channels_last:
            return self.final_conv(x)
        B, C = x.shape[:2]
        w = self.final_conv.weight.reshape(self.final_conv.out_channels, C)
        y = torch.baddbmm(self.final_conv.bias.view(1, 1, -1), x.flatten(2).transpose(1, 2), w.t().unsqueeze(0).expand(B, -1, -1))
        return y.view(B, *x.shape[2:], -1).permute(0, 4, 1, 2, 3)


# ---------------------------------------------------------------------------------------------------------------------
# Point-cloud encoder of the reference's default configuration (generators/pointnet.py:59-180; dataset.load_pcl): a PointNet with
# fully connected residual blocks turns a cloud (B, T, dim) -- xyz and rgb: dim = 6 -- into one latent per object, which drives
# the FiLM mapping network of SHORTSIREN.  Stock PyTorch: a dozen small GEMMs.  Module names are the reference's, so the
# `encoder_state_dict` of its checkpoints loads.
# ---------------------------------------------------------------------------------------------------------------------
class ResnetBlockFC(nn.Module):
    """x -> shortcut(x) + fc_1(relu(fc_0(relu(x)))); the shortcut is a bias-free Linear when the widths differ; fc_1 starts at zero."""

    def __init__(self, size_in, size_out=None, size_h=None):
        super().__init__()
        size_out = size_in if size_out is None else size_out
        size_h = min(size_in, size_out) if size_h is None else size_h
        self.size_in, self.size_h, self.size_out = size_in, size_h, size_out
        self.fc_0 = nn.Linear(size_in, size_h)
        self.fc_1 = nn.Linear(size_h, size_out)
        self.actvn = nn.ReLU()
        self.shortcut = None if size_in == size_out else nn.Linear(size_in, size_out, bias=False)
        nn.init.zeros_(self.fc_1.weight)

    def forward(self, x):
        dx = self.fc_1(self.actvn(self.fc_0(self.actvn(x))))
        return (x if self.shortcut is None else self.shortcut(x)) + dx


class ResnetPointnet(nn.Module):
    """(B, T, dim) -> (B, c_dim).  Five residual blocks of width 2 h -> h; between them every point's features are joined with
    the maximum over the cloud's points; the last block's output is max-pooled over the points and projected by fc_c."""

    def __init__(self, c_dim=512, dim=3, hidden_dim=512):
        super().__init__()
        self.c_dim = c_dim
        self.fc_pos = nn.Linear(dim, 2 * hidden_dim)
        for i in range(5):
            setattr(self, f"block_{i}", ResnetBlockFC(2 * hidden_dim, hidden_dim))
        self.fc_c = nn.Linear(hidden_dim, c_dim)
        self.actvn = nn.ReLU()

    def forward(self, p):
        net = self.block_0(self.fc_pos(p))
        for i in range(1, 5):
            pooled = net.max(dim=1, keepdim=True)[0].expand_as(net)
            net = getattr(self, f"block_{i}")(torch.cat([net, pooled], dim=2))
        return self.fc_c(self.actvn(net.max(dim=1)[0]))


def encode_pcl(encoder, pcl, device, noise_weight=0):
    """-> (z, l_reg): the encoder's latents, each row normalised to zero mean and unit (unbiased) standard deviation and mixed
    with Gaussian noise, z = noise_weight * randn + (1 - noise_weight) * normalised; l_reg is the mean row norm of the latents
    BEFORE the normalisation (the G step's regulariser, utils.py:694-706)."""
    codes = encoder(pcl.to(device))
    l_reg = codes.norm(dim=1).mean()
    normalised = codes - codes.mean(dim=1, keepdim=True)
    normalised = normalised / normalised.std(dim=1, keepdim=True)
    noise = torch.randn(normalised.shape, device=device)
    return noise_weight * noise + (1 - noise_weight) * normalised, l_reg
