"""fp32 CPU restatement of torchvision's ``raft_large`` (models/optical_flow/raft.py) in plain torch — the yardstick of the native
estimator (univst_amd/flow.py, csrc/raft.hip).  A helper module, not a conftest.

Written from the published definition: the module tree and the state-dict keys are torchvision's, so ``load_state_dict(strict=True)``
works in both directions.  ``round_fp16=True`` rounds the weights and every conv input and output to fp16 (what the native path's fp16
convs with fp32 accumulation do); everything else — norms, correlation volume, lookups, coordinates, GRU state — stays fp32.
The stages are separate functions: ``build_pyramid``, ``index_pyramid``, ``gru``, ``upsample_flow``."""
import torch
import torch.nn as nn
import torch.nn.functional as F


def _r16(t):
    return t.half().float()


class Conv(nn.Conv2d):
    """Conv2d whose fp16 switch (set by RAFT.set_round_fp16) rounds weight, bias, input and output to fp16; arithmetic stays fp32"""
    round_fp16 = False

    def forward(self, x):
        if not self.round_fp16:
            return super().forward(x)
        b = None if self.bias is None else _r16(self.bias)
        return _r16(F.conv2d(_r16(x), _r16(self.weight), b, self.stride, self.padding))


class ConvNormAct(nn.Sequential):
    """torchvision Conv2dNormActivation: conv at .0, norm at .1 (when there is one), then ReLU (when there is one)"""

    def __init__(self, cin, cout, kernel_size, stride=1, norm_layer=None, relu=True):
        layers = [Conv(cin, cout, kernel_size, stride, (kernel_size - 1) // 2, bias=True)]
        if norm_layer is not None:
            layers.append(norm_layer(cout))
        if relu:
            layers.append(nn.ReLU())
        super().__init__(*layers)


class ResidualBlock(nn.Module):
    def __init__(self, cin, cout, norm_layer, stride=1):
        super().__init__()
        self.convnormrelu1 = ConvNormAct(cin, cout, 3, stride, norm_layer)
        self.convnormrelu2 = ConvNormAct(cout, cout, 3, 1, norm_layer)
        self.downsample = nn.Identity() if stride == 1 else ConvNormAct(cin, cout, 1, stride, norm_layer, relu=False)

    def forward(self, x):
        y = self.convnormrelu2(self.convnormrelu1(x))
        return torch.relu(self.downsample(x) + y)


class Encoder(nn.Module):
    def __init__(self, norm_layer, layers=(64, 64, 96, 128, 256)):
        super().__init__()
        self.convnormrelu = ConvNormAct(3, layers[0], 7, 2, norm_layer)
        self.layer1 = nn.Sequential(ResidualBlock(layers[0], layers[1], norm_layer, 1), ResidualBlock(layers[1], layers[1], norm_layer, 1))
        self.layer2 = nn.Sequential(ResidualBlock(layers[1], layers[2], norm_layer, 2), ResidualBlock(layers[2], layers[2], norm_layer, 1))
        self.layer3 = nn.Sequential(ResidualBlock(layers[2], layers[3], norm_layer, 2), ResidualBlock(layers[3], layers[3], norm_layer, 1))
        self.conv = Conv(layers[3], layers[4], 1)

    def forward(self, x):
        return self.conv(self.layer3(self.layer2(self.layer1(self.convnormrelu(x)))))


class MotionEncoder(nn.Module):
    def __init__(self):
        super().__init__()
        self.convcorr1 = ConvNormAct(324, 256, 1)
        self.convcorr2 = ConvNormAct(256, 192, 3)
        self.convflow1 = ConvNormAct(2, 128, 7)
        self.convflow2 = ConvNormAct(128, 64, 3)
        self.conv = ConvNormAct(256, 126, 3)

    def forward(self, flow, corr_features):
        corr = self.convcorr2(self.convcorr1(corr_features))
        fl = self.convflow2(self.convflow1(flow))
        return torch.cat([self.conv(torch.cat([corr, fl], dim=1)), flow], dim=1)


class ConvGRU(nn.Module):
    def __init__(self, kernel_size, padding):
        super().__init__()
        self.convz = Conv(384, 128, kernel_size, padding=padding)
        self.convr = Conv(384, 128, kernel_size, padding=padding)
        self.convq = Conv(384, 128, kernel_size, padding=padding)

    def forward(self, h, x):
        hx = torch.cat([h, x], dim=1)
        z = torch.sigmoid(self.convz(hx))
        r = torch.sigmoid(self.convr(hx))
        q = torch.tanh(self.convq(torch.cat([r * h, x], dim=1)))
        return (1 - z) * h + z * q


class RecurrentBlock(nn.Module):
    def __init__(self):
        super().__init__()
        self.convgru1 = ConvGRU((1, 5), (0, 2))
        self.convgru2 = ConvGRU((5, 1), (2, 0))

    def forward(self, h, x):
        return self.convgru2(self.convgru1(h, x), x)


class FlowHead(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = Conv(128, 256, 3, padding=1)
        self.conv2 = Conv(256, 2, 3, padding=1)

    def forward(self, x):
        return self.conv2(torch.relu(self.conv1(x)))


class UpdateBlock(nn.Module):
    def __init__(self):
        super().__init__()
        self.motion_encoder = MotionEncoder()
        self.recurrent_block = RecurrentBlock()
        self.flow_head = FlowHead()

    def forward(self, hidden, context, corr_features, flow):
        motion = self.motion_encoder(flow, corr_features)
        hidden = self.recurrent_block(hidden, torch.cat([context, motion], dim=1))
        return hidden, self.flow_head(hidden)


class MaskPredictor(nn.Module):
    def __init__(self):
        super().__init__()
        self.convrelu = ConvNormAct(128, 256, 3)
        self.conv = Conv(256, 576, 1)

    def forward(self, x):
        return 0.25 * self.conv(self.convrelu(x))


# ---------------------------------------------------------------------------------------------------------------- stages
def build_pyramid(fmap1, fmap2, num_levels=4):
    """fmaps [B, C, h, w] -> list of [B*h*w, 1, h >> l, w >> l]: all-pairs correlation / sqrt(C), then 2x2 average pooling (floor)"""
    b, c, h, w = fmap1.shape
    corr = torch.matmul(fmap1.reshape(b, c, h * w).transpose(1, 2), fmap2.reshape(b, c, h * w)) / (c ** 0.5)
    corr = corr.reshape(b * h * w, 1, h, w)
    pyramid = [corr]
    for _ in range(num_levels - 1):
        corr = F.avg_pool2d(corr, kernel_size=2, stride=2)
        pyramid.append(corr)
    return pyramid


def grid_sample(img, absolute_grid):
    """torchvision's wrapper: absolute pixel coordinates, bilinear, align_corners=True, zeros outside"""
    h, w = img.shape[-2:]
    xg, yg = absolute_grid.split([1, 1], dim=-1)
    xg = 2 * xg / (w - 1) - 1
    yg = 2 * yg / (h - 1) - 1
    return F.grid_sample(img, torch.cat([xg, yg], dim=-1), mode="bilinear", align_corners=True)


def index_pyramid(pyramid, centroids_coords, radius=4):
    """centroids [B, 2, h, w] (x, y) -> [B, levels * 81, h, w]; channel l*81 + a*9 + b samples level l at x / 2^l + (a - 4), y / 2^l + (b - 4)"""
    side = 2 * radius + 1
    di = torch.linspace(-radius, radius, side)
    dj = torch.linspace(-radius, radius, side)
    delta = torch.stack(torch.meshgrid(di, dj, indexing="ij"), dim=-1).view(1, side, side, 2)
    b, _, h, w = centroids_coords.shape
    cen = centroids_coords.permute(0, 2, 3, 1).reshape(b * h * w, 1, 1, 2)
    out = []
    for corr in pyramid:
        out.append(grid_sample(corr, cen + delta).view(b, h, w, -1))
        cen = cen / 2
    return torch.cat(out, dim=-1).permute(0, 3, 1, 2).contiguous()


def gru(recurrent_block, hidden, context, motion):
    """one RecurrentBlock step on [B, 128, h, w] tensors"""
    return recurrent_block(hidden, torch.cat([context, motion], dim=1))


def upsample_flow(flow, up_mask, factor=8):
    """flow [B, 2, h, w], up_mask [B, 576, h, w] (already times 0.25) -> [B, 2, 8h, 8w]"""
    b, c, h, w = flow.shape
    m = torch.softmax(up_mask.view(b, 1, 9, factor, factor, h, w), dim=2)
    up = F.unfold(factor * flow, kernel_size=3, padding=1).view(b, c, 9, 1, 1, h, w)
    up = torch.sum(m * up, dim=2)
    return up.permute(0, 1, 4, 2, 5, 3).reshape(b, c, h * factor, w * factor)


def make_coords_grid(b, h, w):
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    return torch.stack([xs, ys], dim=0).float()[None].repeat(b, 1, 1, 1)


class RAFT(nn.Module):
    """raft_large: forward(image1, image2) with [B, 3, H, W] float images -> list of the 12 upsampled flows [B, 2, H, W] (torchvision's return value)"""

    def __init__(self, round_fp16=False):
        super().__init__()
        self.feature_encoder = Encoder(nn.InstanceNorm2d)
        self.context_encoder = Encoder(nn.BatchNorm2d)
        self.update_block = UpdateBlock()
        self.mask_predictor = MaskPredictor()
        self.set_round_fp16(round_fp16)

    def set_round_fp16(self, on):
        for m in self.modules():
            if isinstance(m, Conv):
                m.round_fp16 = bool(on)
        return self

    def encode(self, image1, image2):
        """-> fmap1, fmap2 [B, 256, h, w], hidden (tanh) and context (relu) [B, 128, h, w]"""
        fmaps = self.feature_encoder(torch.cat([image1, image2], dim=0))
        fmap1, fmap2 = torch.chunk(fmaps, 2, dim=0)
        hidden, context = torch.split(self.context_encoder(image1), [128, 128], dim=1)
        return fmap1, fmap2, torch.tanh(hidden), torch.relu(context)

    @torch.no_grad()
    def forward(self, image1, image2, num_flow_updates=12):
        b, _, h, w = image1.shape
        if not (h % 8 == 0 and w % 8 == 0):
            raise ValueError(f"input image H and W should be divisible by 8, but got {h} (h) and {w} (w)")
        fmap1, fmap2, hidden, context = self.encode(image1, image2)
        if min(fmap1.shape[-2:]) < 16:
            raise ValueError("Feature maps are too small to be down-sampled by the correlation pyramid.")
        pyramid = build_pyramid(fmap1, fmap2)
        coords0 = make_coords_grid(b, h // 8, w // 8)
        coords1 = make_coords_grid(b, h // 8, w // 8)
        flows = []
        for _ in range(num_flow_updates):
            corr_features = index_pyramid(pyramid, coords1)
            hidden, delta = self.update_block(hidden, context, corr_features, coords1 - coords0)
            coords1 = coords1 + delta
            flows.append(upsample_flow(coords1 - coords0, self.mask_predictor(hidden)))
        self.last_lowres_flow = coords1 - coords0
        return flows


def random_state_dict(seed=0, gain=1.0, head_gain=1.0):
    """a seeded random raft_large state dict: default torch initialisation of every conv scaled by `gain` (`head_gain` for the flow head's last
    conv, which sets the size of the flow), BatchNorm statistics away from (0, 1) so that the fold is exercised"""
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    m = RAFT()
    sd = m.state_dict()
    for k, v in sd.items():
        if k.endswith("running_mean"):
            v.copy_(torch.randn(v.shape, generator=g) * 0.1)
        elif k.endswith("running_var"):
            v.copy_(torch.rand(v.shape, generator=g) * 0.5 + 0.75)
        elif k.endswith(".1.weight"):
            v.copy_(torch.rand(v.shape, generator=g) * 0.5 + 0.75)
        elif k.endswith(".1.bias"):
            v.copy_(torch.randn(v.shape, generator=g) * 0.1)
        elif v.dtype.is_floating_point:
            v.mul_(head_gain if k.startswith("update_block.flow_head.conv2") else gain)
    return sd


def make_images(H, W, seed=0, shift=(3, 2)):
    """a smooth random texture and a shifted, slightly perturbed copy, uint8 [H, W, 3]"""
    g = torch.Generator().manual_seed(seed)
    base = F.interpolate(torch.rand(1, 3, H // 4 + 8, W // 4 + 8, generator=g), scale_factor=4, mode="bicubic", align_corners=False)[0]
    a = base[:, 8:8 + H, 8:8 + W]
    b = base[:, 8 - shift[1]:8 - shift[1] + H, 8 - shift[0]:8 - shift[0] + W] + 0.02 * torch.randn(3, H, W, generator=g)
    to8 = lambda t: (t.clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous()
    return to8(a), to8(b)


def preprocess(img_u8):
    """preprocess_image of the reference's src/cal_optica_flow.py: HWC uint8 -> [1, 3, H, W] float in [0, 1]"""
    return img_u8.permute(2, 0, 1).float().unsqueeze(0) / 255.0
