"""Frechet distance between two sets of feature vectors (the distance part of src/fid.py:95-163) and a labelled PROXY of
the reference's FID.

The reference's FID extracts pool features with a pretrained Inception-v3 (src/fid.py:32-93); those weights cannot be
obtained offline, so ``fid_proxy`` uses the DISCRIMINATOR's trunk as the feature extractor (the activation in front of its
head, spatially averaged to (N, C) exactly as the reference averages Inception's Mixed_7c map, eval-mode BatchNorm) and
says so in its name.  The statistics and the distance are the reference's: mu = mean, sigma = np.cov(rowvar=False);
d^2 = |mu1 - mu2|^2 + Tr(C1 + C2 - 2 (C1 C2)^(1/2)) with the matrix square root from scipy and the usual remedies for a
(near-)singular product (add eps to the diagonals) and for a small imaginary part from round-off.
"""
from __future__ import annotations

import warnings

import numpy as np
import torch
from scipy import linalg


def activation_statistics(act):
    """(mu, sigma) of an (N, F) array of feature vectors (src/fid.py:106-109)."""
    act = np.asarray(act, dtype=np.float64)
    return act.mean(axis=0), np.cov(act, rowvar=False)


def frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """Squared Frechet distance between N(mu1, sigma1) and N(mu2, sigma2) (src/fid.py:112-163)."""
    mu1, mu2 = np.atleast_1d(mu1), np.atleast_1d(mu2)
    sigma1, sigma2 = np.atleast_2d(sigma1), np.atleast_2d(sigma2)
    if mu1.shape != mu2.shape or sigma1.shape != sigma2.shape:
        raise ValueError("the two sets of statistics have different dimensions")
    delta = mu1 - mu2
    root, _ = linalg.sqrtm(sigma1.dot(sigma2), disp=False)
    if not np.isfinite(root).all():          # singular product: regularise both covariances
        warnings.warn("frechet_distance: singular covariance product; adding %g to the diagonals" % eps)
        jitter = np.eye(sigma1.shape[0]) * eps
        root = linalg.sqrtm((sigma1 + jitter).dot(sigma2 + jitter))
    if np.iscomplexobj(root):                # round-off can leave a tiny imaginary part
        if not np.allclose(np.diagonal(root).imag, 0, atol=1e-3):
            raise ValueError("frechet_distance: imaginary component %g" % np.max(np.abs(root.imag)))
        root = root.real
    return float(delta.dot(delta) + np.trace(sigma1) + np.trace(sigma2) - 2.0 * np.trace(root))


@torch.no_grad()
def discriminator_features(discriminator, images, batch_size=64):
    """(N, C) features: the discriminator trunk's last activation (eval-mode BatchNorm), averaged over its 4x4 map.
    ``images``: (N, 3, S, S) float tensor in [-1, 1] (the GAN's own normalisation)."""
    was_training = discriminator.training
    discriminator.eval()
    dev = next(discriminator.parameters()).device
    feats = []
    try:
        for i in range(0, images.shape[0], batch_size):
            f = discriminator(images[i:i + batch_size].to(dev).float(), feature_matching=True)
            feats.append(f.mean(dim=(2, 3)).cpu().numpy())
    finally:
        discriminator.train(was_training)
    return np.concatenate(feats, axis=0)


def fid_proxy(discriminator, images1, images2, batch_size=64):
    """Frechet distance between the discriminator-trunk features of two image sets.  NOT the Inception FID of
    src/fid.py:217-232 (no Inception weights offline): comparable only between runs that use the same discriminator."""
    m1, s1 = activation_statistics(discriminator_features(discriminator, images1, batch_size))
    m2, s2 = activation_statistics(discriminator_features(discriminator, images2, batch_size))
    return frechet_distance(m1, s1, m2, s2)


# ------------------------------------------------------------------------------------------------------------------
# The rest of the reference's FID procedure around the feature extractor (src/fid.py:166-232, :312-330).  The extractor
# itself (Inception-v3 Mixed_7c pool features, :33-94) needs pretrained weights that are not obtainable offline, so it
# is a parameter here: any callable (N, 3, 299, 299) float tensor in [0, 1] -> (N, F) array.
# ------------------------------------------------------------------------------------------------------------------
def preprocess_image(im):
    """src/fid.py:166-190: (H, W, 3) uint8 or float32 in [0, 1] -> (3, 299, 299) float32 in [0, 1].  The reference
    resizes with cv2.resize(im, (299, 299)) (bilinear, half-pixel centres, no anti-aliasing); cv2 is absent here, the
    same sampling rule is applied with torch (parity with cv2 unpinned: no cv2 to compare with)."""
    im = np.asarray(im)
    if im.ndim != 3 or im.shape[2] != 3:
        raise ValueError("preprocess_image expects an (H, W, 3) image")
    if im.dtype == np.uint8:
        im = im.astype(np.float32) / 255
    t = torch.from_numpy(np.ascontiguousarray(im, dtype=np.float32)).permute(2, 0, 1)[None]
    t = torch.nn.functional.interpolate(t, size=(299, 299), mode="bilinear", align_corners=False, antialias=False)[0]
    if float(t.max()) > 1.0 or float(t.min()) < 0.0:
        raise ValueError("preprocess_image: values outside [0, 1]")
    return t.contiguous()


def preprocess_images(images, use_multiprocessing=False):
    """src/fid.py:193-214: (N, H, W, 3) -> (N, 3, 299, 299) float32 in [0, 1] (use_multiprocessing is accepted for
    signature compatibility; the resize is a single batched op here)."""
    out = torch.stack([preprocess_image(im) for im in images], dim=0)
    assert out.shape == (len(images), 3, 299, 299) and out.dtype == torch.float32
    return out


def calculate_fid(images1, images2, feature_extractor, batch_size=2, use_multiprocessing=False, on_device=False):
    """src/fid.py:217-232 with the feature extractor as a parameter: images (N, H, W, 3) uint8 / float in [0, 1].
    on_device=True: each set is uploaded once (as uint8 / fp32) and resize, features and moments run on the device
    (fid_statistics_device; ``feature_extractor`` must then return device tensors, e.g. inception_features_device); only the
    distance is computed on the host."""
    if on_device:
        m1, s1, _ = fid_statistics_device(images1, feature_extractor, batch_size)
        m2, s2, _ = fid_statistics_device(images2, feature_extractor, batch_size)
        return frechet_distance(m1, s1, m2, s2)

    def feats(images):
        x = preprocess_images(images, use_multiprocessing)
        return np.concatenate([np.asarray(feature_extractor(x[i:i + batch_size]), dtype=np.float64)
                               for i in range(0, x.shape[0], batch_size)], axis=0)
    m1, s1 = activation_statistics(feats(images1))
    m2, s2 = activation_statistics(feats(images2))
    return frechet_distance(m1, s1, m2, s2)


def inception_feature_extractor(weights, device="cuda:0"):
    """The reference's feature extractor (src/fid.py:33-94: torchvision inception_v3 up to Mixed_7c, spatially averaged) on
    the HIP kernels, as the ``feature_extractor`` argument of calculate_fid / fid_protocol.  ``weights``: a torchvision
    ``inception_v3`` state_dict (or the path of a file holding one) -- pretrained weights are not obtainable offline, they
    are an input here.  Returns a callable (N, 3, 299, 299) float tensor in [0, 1] -> (N, 2048) float32 array."""
    from .inception import InceptionV3
    net = InceptionV3()
    if isinstance(weights, (str, bytes)):
        weights = torch.load(weights, map_location="cpu")
    net.load_state_dict(weights)
    net = net.to(device).eval()

    def extract(x01):
        return net.features(x01.to(device)).cpu().numpy()
    return extract


def fid_protocol(generate_fake, real_images, feature_extractor, iterations=5, batch_size=2, on_device=False):
    """The reference's reporting protocol (src/fid.py:312-330): `iterations` (= 5) independent generations of the fake
    set against the same real set, FID of each, reported as mean +- std.  generate_fake() -> (N, H, W, 3) images.
    on_device: as calculate_fid."""
    values = [calculate_fid(real_images, generate_fake(), feature_extractor, batch_size, on_device=on_device)
              for _ in range(iterations)]
    return {"fid_values": values, "mean": float(np.mean(values)), "std": float(np.std(values))}


# ------------------------------------------------------------------------------------------------------------------
# The same protocol without the host in the loop: images that are already on the device (the generator's output, a real
# set uploaded once) are resized by rg_resize_bilinear01, go through a device-side extractor, and only the features' raw
# moments -- F + F^2 doubles, accumulated by rg_moments_update -- come back.
# ------------------------------------------------------------------------------------------------------------------
_RANGE_MAPS = {(0.0, 1.0): (1.0, 0.0), (-1.0, 1.0): (0.5, 0.5)}     # value range -> (mul, add) of the fp32 tap


def _image_layout(images, layout):
    if images.dim() != 4:
        raise ValueError("expected a 4-d image batch, got shape %s" % (tuple(images.shape),))
    if layout is None:
        nchw, nhwc = images.shape[1] == 3, images.shape[3] == 3
        if nchw == nhwc:
            raise ValueError("cannot tell (N, 3, H, W) from (N, H, W, 3) for shape %s: pass layout='NCHW' or 'NHWC'"
                             % (tuple(images.shape),))
        layout = "NCHW" if nchw else "NHWC"
    if layout not in ("NCHW", "NHWC"):
        raise ValueError("layout must be 'NCHW' or 'NHWC'")
    return layout


def preprocess_images_device(images, size=299, value_range=None, layout=None):
    """Device counterpart of preprocess_images: (N, 3, size, size) fp32 in [0, 1] ON THE DEVICE from ONE launch of
    rg_resize_bilinear01 (bilinear, half-pixel centres, no anti-aliasing), strides taken from the tensor (no copy, a slice
    of a larger batch included).  ``images``: a device tensor,
      uint8 (N, 3, H, W) or (N, H, W, 3)                       -- tap v / 255;
      fp32  with value_range=(-1, 1), e.g. (N, 3, H, W) from the generator  -- tap v * 0.5 + 0.5;
      fp32  with value_range=(0, 1), e.g. (N, H, W, 3) from generate_images -- tap v.
    The value range of an fp32 batch is a keyword, never guessed from the data; the layout is told by which axis is 3
    (``layout`` settles H = 3 or W = 3).
    NOT bit-identical to preprocess_images: torch's interpolate computes source coordinates in fp32, this kernel in fp64
    (the weights are then rounded to fp32).  The difference is at most 4 ulp_fp32(max(H, W)) -- two axes x two roundings of
    an fp32 coordinate x tap differences <= 1 -- i.e. 6.1e-5 at 256; measured 1.4e-5 at 256 -> 299, 2.3e-5 at 512 -> 299
    (tests/test_fid_device_refs_cpu.py)."""
    from . import _abi
    if not (torch.is_tensor(images) and images.is_cuda):
        raise TypeError("preprocess_images_device takes a tensor on the GPU (preprocess_images is the host path)")
    layout = _image_layout(images, layout)
    if images.dtype == torch.uint8:
        dtype, (mul, add) = _abi.RG_U8, (1.0, 0.0)
    elif images.dtype == torch.float32:
        key = None if value_range is None else (float(value_range[0]), float(value_range[1]))
        if key not in _RANGE_MAPS:
            raise ValueError("an fp32 batch needs value_range=(0, 1) or (-1, 1), got %r" % (value_range,))
        dtype, (mul, add) = _abi.RG_F32, _RANGE_MAPS[key]
    else:
        raise TypeError("preprocess_images_device takes uint8 or float32 images, got %s" % images.dtype)
    if layout == "NCHW":
        N, C, H, W = images.shape
        sn, sc, sh, sw = images.stride()
    else:
        N, H, W, C = images.shape
        sn, sh, sw, sc = images.stride()
    if C != 3:
        raise ValueError("expected 3 channels, got %d" % C)
    size = int(size)
    out = torch.empty((N, 3, size, size), dtype=torch.float32, device=images.device)
    _abi.launch("rg_resize_bilinear01", images.device, images.data_ptr(), dtype, sn, sc, sh, sw, mul, add, out.data_ptr(), N, 3, H, W,
                size, size)
    return out


class FeatureMoments:
    """Running first and second raw moments of (n, F) fp32 feature rows, kept on the device in fp64 by rg_moments_update
    (exact products, one deterministic chain of additions per entry); ``statistics()`` downloads F + F^2 doubles and finishes
    (mu, sigma) on the host with np.cov's normalisation."""

    def __init__(self, F, device):
        self.F = int(F)
        if self.F < 1:
            raise ValueError("FeatureMoments: F must be >= 1")
        self.device = torch.device(device)
        self.s1 = torch.zeros(self.F, dtype=torch.float64, device=self.device)
        self.s2 = torch.zeros(self.F, self.F, dtype=torch.float64, device=self.device)
        self.n = 0

    def update(self, feats):
        from . import _abi
        if not (torch.is_tensor(feats) and feats.is_cuda and feats.dtype == torch.float32 and feats.dim() == 2):
            raise TypeError("FeatureMoments.update takes an (n, F) float32 tensor on the GPU")
        if feats.shape[1] != self.F or feats.device != self.s1.device:
            raise ValueError("FeatureMoments.update: expected (n, %d) on %s, got %s on %s"
                             % (self.F, self.s1.device, tuple(feats.shape), feats.device))
        if feats.stride(1) != 1 or (feats.shape[0] > 1 and feats.stride(0) < self.F):
            feats = feats.contiguous()
        n = feats.shape[0]
        ldx = feats.stride(0) if n > 1 else self.F
        _abi.launch("rg_moments_update", self.s1.device, feats.data_ptr(), ldx, n, self.F, self.s1.data_ptr(), self.s2.data_ptr())
        self.n += n
        return self

    @staticmethod
    def finish(s1, s2, n):
        """(mu, sigma) from the raw moments of n rows: mu = s1 / n, sigma = (s2 - n mu mu^T) / (n - 1)  (np.cov's divisor)."""
        if n < 2:
            raise ValueError("a covariance needs at least 2 feature rows, got %d" % n)
        s1, s2 = np.asarray(s1, dtype=np.float64), np.asarray(s2, dtype=np.float64)
        mu = s1 / n
        return mu, (s2 - n * np.outer(mu, mu)) / (n - 1)

    def statistics(self):
        if self.n < 2:
            raise ValueError("a covariance needs at least 2 feature rows, got %d" % self.n)
        return self.finish(self.s1.cpu().numpy(), self.s2.cpu().numpy(), self.n)


def discriminator_features_device(discriminator):
    """Device-side extractor of the labelled PROXY (see fid_proxy): images (n, 3, S, S) fp32 in [-1, 1] on the device ->
    (n, C) features on the device.  The same eval-mode trunk forward and the same mean(dim=(2, 3)) as
    discriminator_features, so a batch gives the same bits as there.  The module's train / eval mode is restored."""
    @torch.no_grad()
    def extract(images):
        was_training = discriminator.training
        discriminator.eval()
        try:
            dev = next(discriminator.parameters()).device
            f = discriminator(images.to(dev).float(), feature_matching=True)
            return f.mean(dim=(2, 3))
        finally:
            discriminator.train(was_training)
    return extract


def inception_features_device(weights, device="cuda:0"):
    """inception_feature_extractor without the copy to the host: (N, 3, 299, 299) fp32 in [0, 1] -> (N, 2048) fp32 on the
    device."""
    from .inception import InceptionV3
    net = InceptionV3()
    if isinstance(weights, (str, bytes)):
        weights = torch.load(weights, map_location="cpu")
    net.load_state_dict(weights)
    net = net.to(device).eval()

    def extract(x01):
        return net.features(x01.to(device))
    return extract


def device_statistics(batches, extractor, resize=None, value_range=None):
    """(mu, sigma, n) of the features of an iterable of device image batches; the features never leave the device.
    resize=299: every batch goes through preprocess_images_device(batch, 299, value_range) first (an Inception extractor);
    resize=None: the batches are handed to ``extractor`` as they are (the discriminator proxy at native resolution).
    ``extractor``: batch -> (n, F) float32 tensor on the device."""
    moments = None
    for batch in batches:
        if resize is not None:
            batch = preprocess_images_device(batch, resize, value_range)
        feats = extractor(batch)
        if not (torch.is_tensor(feats) and feats.is_cuda):
            raise TypeError("device_statistics needs an extractor that returns device tensors (discriminator_features_device, "
                            "inception_features_device); a host extractor belongs to calculate_fid(on_device=False)")
        feats = feats.float()
        if moments is None:
            moments = FeatureMoments(feats.shape[1], feats.device)
        moments.update(feats)
    if moments is None:
        raise ValueError("device_statistics: no batches")
    mu, sigma = moments.statistics()
    return mu, sigma, moments.n


def device_features(batches, extractor, resize=None, value_range=None):
    """device_statistics' loop and checks, returning the features themselves: the (n, F) fp32 features of an iterable of device
    image batches as ONE contiguous device tensor (what rna_gan_amd.kid's Gram sums read; nothing goes to the host)."""
    feats = []
    for batch in batches:
        if resize is not None:
            batch = preprocess_images_device(batch, resize, value_range)
        f = extractor(batch)
        if not (torch.is_tensor(f) and f.is_cuda):
            raise TypeError("device_features needs an extractor that returns device tensors (discriminator_features_device, "
                            "inception_features_device)")
        if f.dim() != 2 or (feats and (f.shape[1] != feats[0].shape[1] or f.device != feats[0].device)):
            raise ValueError("device_features: the extractor returned %s after %s" % (
                tuple(f.shape), tuple(feats[0].shape) if feats else "nothing"))
        feats.append(f.float())
    if not feats:
        raise ValueError("device_features: no batches")
    return torch.cat(feats, dim=0).contiguous()


def _device_image_set(images, device=None):
    """host (N, H, W, 3) uint8 / float in [0, 1] images (or a device tensor of that form), uploaded once: uint8 or fp32"""
    if torch.is_tensor(images):
        x = images
    else:
        x = np.asarray(images)
        if x.dtype != np.uint8:
            x = x.astype(np.float32, copy=False)
        x = torch.from_numpy(np.ascontiguousarray(x))
    if x.dim() != 4 or x.shape[3] != 3:
        raise ValueError("expected (N, H, W, 3) images")
    if not x.is_cuda:
        x = x.to(device if device is not None else "cuda:0")
    if x.dtype != torch.uint8:
        x = x.float()
    return x


def device_feature_pair(images1, images2, feature_extractor, batch_size=2, device=None):
    """the two (N, F) fp32 device feature sets of kid.calculate_kid and prdc.calculate_prdc: each image set (as
    _device_image_set takes it) is uploaded once, then resized to 299 and extracted on the device"""
    sets = (_device_image_set(images, device) for images in (images1, images2))
    return tuple(device_features((x[i:i + batch_size] for i in range(0, x.shape[0], batch_size)), feature_extractor, resize=299,
                                 value_range=(0, 1)) for x in sets)


def fid_statistics_device(images, feature_extractor, batch_size=2, device=None):
    """(mu, sigma, n) of calculate_fid(on_device=True) for ONE image set: host (N, H, W, 3) uint8 / float in [0, 1] images
    (or a device tensor of that form) are uploaded once, then resized to 299, extracted and accumulated on the device."""
    x = _device_image_set(images, device)
    return device_statistics((x[i:i + batch_size] for i in range(0, x.shape[0], batch_size)), feature_extractor, resize=299,
                             value_range=(0, 1))
