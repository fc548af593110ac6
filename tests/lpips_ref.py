"""Yardstick of binocular3dgs_amd/lpips.py: the network and the taps of lpipsPyTorch written with torch on the CPU, in float64
by default, from the formulae of the reference:

    modules/networks.py:50-63   z_score (x - mean) / std, layers in order, taps after target layers
    modules/networks.py:88-96   VGG16: torchvision's vgg16().features, target layers 4, 9, 16, 23, 30 = relu1_2 .. relu5_3
    modules/utils.py:6-8        normalize_activation: x / (sqrt(sum_c x^2) + 1e-10)
    modules/lpips.py:30-36      (fx - fy)^2, the 1x1 `lin` convolution, mean over (H, W), sum over the layers

The reference's own module needs torchvision and a download, neither of which a test may rely on, so there is no golden file:
these few lines are the statement.  `dtype=torch.float32` runs the same lines in float32 (the tolerance of the device test is
measured from the difference)."""
import torch
import torch.nn.functional as F

from binocular3dgs_amd.lpips import TAP_AFTER


def features(x, w, normalize=False, dtype=torch.float64):
    """x: [n,3,H,W] on the CPU; w: lpips.LpipsWeights -> the five tap feature maps (before normalize_activation)."""
    x = x.detach().cpu().to(dtype)
    if normalize:
        x = 2 * x - 1
    shift = torch.tensor(w.shift, dtype=torch.float32).to(dtype)[None, :, None, None]
    scale = torch.tensor(w.scale, dtype=torch.float32).to(dtype)[None, :, None, None]
    x = (x - shift) / scale
    out = []
    for i in range(13):
        if i in (2, 4, 7, 10):
            x = F.max_pool2d(x, kernel_size=2, stride=2)          # torchvision's MaxPool2d(2, 2): floor mode
        x = F.relu(F.conv2d(x, w.conv_w[i].to(dtype), w.conv_b[i].to(dtype), stride=1, padding=1))
        if i in TAP_AFTER:
            out.append(x)
    return out


def normalize_activation(x, eps=1e-10):
    return x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + eps)


def tap(fx, fy, lin):
    """One layer's term of every pair: [n]."""
    d = (normalize_activation(fx) - normalize_activation(fy)) ** 2
    return (d * lin.to(d.dtype)[None, :, None, None]).sum(1).mean((1, 2))


def lpips_layers(x, y, w, normalize=False, dtype=torch.float64):
    """-> [n,5] of `dtype`: the per-layer terms; LPIPS is their sum over the layers."""
    fx, fy = features(x, w, normalize, dtype), features(y, w, normalize, dtype)
    return torch.stack([tap(a, b, lin) for a, b, lin in zip(fx, fy, w.lin)], 1)


def lpips(x, y, w, normalize=False, dtype=torch.float64):
    return lpips_layers(x, y, w, normalize, dtype).sum(1)
