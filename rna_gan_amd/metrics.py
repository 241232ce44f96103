"""Evaluation metrics of the torchgan ``Trainer`` interface (``Trainer(models, losses_list, metrics_list=[...])``).

torchgan is third-party and its source is absent from the reference tree, so ``EvaluationMetric`` is torchgan's interface AS
RECALLED (like the rest of the trainer): a metric has an ``arg_map`` that may rename the trainer
attributes its ``metric_ops`` takes, ``set_arg_map``, ``preprocess``, ``calculate_score`` and ``metric_ops(...)``, which the
trainer calls once per epoch with arguments resolved BY NAME and whose value it appends to ``metric_logs[<class name>]``.

``FrechetDistance`` is the per-epoch quality signal on top of rna_gan_amd.fid's device path: generated images never leave
the device, an evaluation moves F + F^2 doubles per image set to the host and computes one F x F matrix square root there.
``KernelDistance`` is the unbiased counterpart on rna_gan_amd.kid: the same two feature sets, three fp64 Gram sums on the device
(rg_polykernel_tile_sums), one double per 64 x 64 tile of row pairs to the host and no matrix function at all.
``PrecisionRecall`` separates what those two distances mix -- fidelity (precision, density) and diversity (recall, coverage) --
by k-nearest-neighbour balls in the same feature space (rna_gan_amd.prdc: rg_knn_radii2, rg_radius_hits); four numbers come back.
``ConditioningFidelity`` asks what none of those can, because they pool the generated set into one cloud: whether the tiles generated
from patient p's expression row look like patient p -- per-patient centroids on the device (rna_gan_amd.representation:
rg_group_sums_update) and the rank of each patient's own real centroid (rg_match_ranks).
``TissueYield`` judges the generated TILES, not features, and needs no real set: the fraction that the reference tiler's acceptance
rule (rna_gan_amd.tissue: tissue mask coverage and contrast, rg_tile_qc) would keep -- the cheap signal for "the generator emits
background".
``Memorisation`` asks the question all of the above answer the wrong way round -- a generator that copies its training tiles
scores BETTER on each of them: the exact nearest training tiles of the generated tiles (rna_gan_amd.nearest: rg_tile_descriptor_i8,
rg_nn_topk_i8) and the fraction that is closer to one than any other training tile is.
``PairDiversity`` asks whether the generated tiles differ from EACH OTHER, in pixel space and without an extractor: the mean MS-SSIM
over fixed random pairs of generated tiles (rna_gan_amd.msssim: rg_msssim_pyramid, rg_msssim_pairs), next to the same figure over
real tiles -- the early sign of mode collapse.
"""
from __future__ import annotations

import contextlib

import torch


@contextlib.contextmanager
def _eval_mode(*modules):
    """the modules in eval mode; on the way out, however it is left, each is put back into the mode it was in"""
    modes = [(m, m.training) for m in modules]
    try:
        for m, _ in modes:
            m.eval()
        yield
    finally:
        for m, was in modes:
            m.train(was)


def feature_extractor(extractor, discriminator, device=None):
    """``(extract, resize)`` of an ``extractor`` setting: "discriminator" -- the discriminator trunk at native resolution (no
    resize); a callable, or the path of a torchvision inception_v3 state dict (loaded onto ``device``) -- behind a resize to
    299 x 299"""
    from . import fid
    if extractor == "discriminator":
        return fid.discriminator_features_device(discriminator), None
    if isinstance(extractor, str):
        extractor = fid.inception_features_device(extractor, device)
    return extractor, 299


def _checked_extractor(extractor):
    if not (extractor == "discriminator" or callable(extractor)):
        raise ValueError("extractor must be 'discriminator' or a callable device-side feature extractor")
    return extractor


def _checked_tiles(tiles, name, rows, least):
    """``tiles`` if it is a (rows >= least, 3, S, S) tensor of uint8 or float tiles"""
    if not torch.is_tensor(tiles) or tiles.dim() != 4 or tiles.shape[1] != 3 or tiles.shape[0] < least:
        raise ValueError("%s must be an (%s, 3, S, S) tensor of tiles" % (name, rows))
    if tiles.dtype != torch.uint8 and not tiles.is_floating_point():
        raise TypeError("%s must be uint8 or float tiles" % name)
    return tiles


class EvaluationMetric:
    """torchgan.metrics.EvaluationMetric (recalled): base class of everything in ``metrics_list``.

    What a metric pickles (the trainer pickles its metrics into every checkpoint) is declared, not written out: a class names
    its ``SETTINGS`` (attributes pickled as they are), what is ``DROPPED`` (data, caches and results: never pickled, None
    after unpickling) and whether it keeps a ``HISTORY`` (``self.history``, one dictionary per evaluation, pickled); the
    declarations of all classes along the MRO add up.  A class that declares no settings pickles as any object does."""

    SETTINGS, DROPPED, HISTORY = (), (), False
    PRIVATE_NOISE = False          # draws from ``self._rng``, a private torch.Generator(self.seed) that is never pickled

    def __init__(self):
        self.arg_map = {}

    @classmethod
    def _declared(cls, what):
        return [name for c in reversed(cls.__mro__) for name in vars(c).get(what, ())]

    def __getstate__(self):
        settings = self._declared("SETTINGS")
        state = {name: getattr(self, name) for name in settings} if settings else dict(self.__dict__)
        state["arg_map"] = dict(self.arg_map)
        if "extractor" in state and not isinstance(state["extractor"], str):
            state["extractor"] = "callable"
        if self.HISTORY:
            state["history"] = [dict(h) for h in self.history]
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        for name in self._declared("DROPPED"):
            setattr(self, name, None)
        if self.HISTORY:
            self.history = [dict(h) for h in state.get("history", [])]
        if self.PRIVATE_NOISE:
            self._rng = torch.Generator().manual_seed(self.seed)

    def adopt_history(self, saved):
        """Go on from the history of ``saved``, this metric as a checkpoint holds it (or None): a copy, dictionary by
        dictionary; the live object keeps everything else."""
        old = getattr(saved, "history", None)
        if isinstance(old, list) and hasattr(self, "history"):
            self.history = [dict(h) for h in old]

    def _record(self, scores, report):
        """One evaluation: ``scores`` kept in ``last`` and, where the class keeps a history, appended to it as a copy; the
        float the trainer logs"""
        self.last = scores
        if self.HISTORY:
            self.history.append(dict(scores))
        return float(scores[report])

    def _require(self, data, what, setter):
        if data is None:
            raise RuntimeError("%s: no %s (an unpickled metric keeps its settings only: call %s)" % (type(self).__name__, what, setter))

    def _real_side(self, attr, compute, fixed):
        """The real set's part of an evaluation, cached in ``attr``: as kept, or ``compute()`` -- which is kept only when
        ``fixed`` (a fixed extractor: it never changes)"""
        value = getattr(self, attr)
        if value is None:
            value = compute()
            if fixed:
                setattr(self, attr, value)
        return value

    def set_arg_map(self, value):
        """Rename arguments of ``metric_ops``: {argument name: trainer attribute name}."""
        self.arg_map.update(value)

    def preprocess(self, x):
        raise NotImplementedError

    def calculate_score(self, x):
        raise NotImplementedError

    def metric_ops(self, generator, discriminator, **kwargs):
        raise NotImplementedError


class _GeneratedSamples(EvaluationMetric):
    """Draws ``n_fake`` generated images from private noise: what every metric that samples the generator shares.  The noise is
    None ((n_fake, E) standard normal values drawn ONCE from a private torch.Generator(seed): at construction when
    ``encoding_dims`` is given, else at the first evaluation from the generator's ``encoding_dims`` -- the same values either
    way), a tensor of n_fake rows, or a callable noise(n) called at every evaluation.  ``count`` names n_fake in the messages
    of the constructor; ``least`` is its smallest value.  ``preprocess`` turns generated images into the uint8 tiles a store
    would hold, in ``LAYOUT``."""

    SETTINGS, DROPPED, PRIVATE_NOISE = ("n_fake", "seed", "batch_size"), ("noise",), True
    LAYOUT = "nhwc"

    def __init__(self, n_fake, noise, seed, batch_size, encoding_dims, count="n_fake", least=1):
        super().__init__()
        self.n_fake = int(n_fake)
        if self.n_fake < least:
            raise ValueError("%s must be >= %d" % (count, least))
        self.seed = int(seed)
        self.batch_size = int(batch_size)
        if self.batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        self._rng = torch.Generator().manual_seed(self.seed)
        if torch.is_tensor(noise) and noise.shape[0] != self.n_fake:
            raise ValueError("noise has %d rows, %s is %d" % (noise.shape[0], count, self.n_fake))
        self.noise = noise
        if noise is None and encoding_dims is not None:
            self.noise = torch.randn(self.n_fake, int(encoding_dims), generator=self._rng)

    def preprocess(self, x):
        """fp32 [-1, 1] NCHW images -> the uint8 tiles a store would hold (the rounding rule), on the device: interleaved RGB,
        or planar -- the training set's layout -- under ``LAYOUT = "nchw"``."""
        from .export import tiles_u8
        return tiles_u8(x.float().contiguous(), layout=self.LAYOUT)

    def _noise_for(self, generator, device):
        if callable(self.noise):
            z = self.noise(self.n_fake)
        else:
            if self.noise is None:
                self.noise = torch.randn(self.n_fake, int(generator.encoding_dims), generator=self._rng)
            z = self.noise
        if z.shape[0] != self.n_fake:
            raise ValueError("noise has %d rows, n_fake is %d" % (z.shape[0], self.n_fake))
        return z.to(device).float()

    def _fake_batches(self, generator, z):
        from .gan_utils import synthesize
        from .models import DCGANGenerator
        for c in torch.split(z, self.batch_size):
            if isinstance(generator, DCGANGenerator):
                yield synthesize(generator, c, chunk=self.batch_size)
            else:
                yield generator(c.contiguous())

    @torch.no_grad()
    def generated_tiles(self, generator, device):
        """The evaluation's uint8 tiles, one device tensor per batch (eval mode, the mode restored); for the metrics whose
        ``preprocess`` turns generated images into tiles."""
        with _eval_mode(generator):
            z = self._noise_for(generator, device)
            return [self.preprocess(img) for img in self._fake_batches(generator, z)]


class _GeneratedAgainstReal(_GeneratedSamples):
    """What FrechetDistance, KernelDistance and PrecisionRecall share: the real set, the batches of both image sets and the
    evaluation frame (eval mode under no_grad, modes restored, the real set's result cached for a fixed extractor).  A subclass
    supplies ``metric_ops`` and what is collected from a set's batches."""

    SETTINGS, DROPPED = ("extractor",), ("real", "_real_stats")

    def __init__(self, real, n_fake=None, extractor="discriminator", noise=None, seed=0, batch_size=256, encoding_dims=None):
        self.extractor = _checked_extractor(extractor)
        self._real_stats = None
        self.real = None
        self.set_real(real)
        super().__init__(self.real.shape[0] if n_fake is None else n_fake, noise, seed, batch_size, encoding_dims, least=2)

    # ------------------------------------------------------------------ data
    def set_real(self, real):
        self.real = _checked_tiles(real, "real", "N >= 2", 2)
        self._real_stats = None

    # ------------------------------------------------------------------ torchgan's hooks
    def preprocess(self, x):
        """A chunk of the real set on the device, in the form its consumer takes: [-1, 1] fp32 for the discriminator (uint8
        tiles through rg_u8_to_norm, the training input transform); unchanged for the resize kernel, which reads uint8."""
        from .representation import _real_batch
        return _real_batch(x, None if self.extractor == "discriminator" else 299, 0.5, 0.5)

    # ------------------------------------------------------------------ evaluation
    def _real_batches(self, device):
        for i in range(0, self.real.shape[0], self.batch_size):
            yield self.preprocess(self.real[i:i + self.batch_size].to(device))

    @torch.no_grad()
    def _collect_sets(self, generator, discriminator, device, collect):
        """(fake, real): ``collect(batches, extract, resize)`` of the generated set and of the real set (the latter kept in
        ``_real_stats`` for a fixed extractor), both networks in eval mode, their modes restored"""
        self._require(self.real, "real set", "set_real")
        with _eval_mode(generator, discriminator):
            extract, resize = feature_extractor(self.extractor, discriminator)
            z = self._noise_for(generator, device)
            fake = collect(self._fake_batches(generator, z), extract, resize)
            return fake, self._real_side("_real_stats", lambda: collect(self._real_batches(device), extract, resize), resize is not None)


class FrechetDistance(_GeneratedAgainstReal):
    """Frechet distance between features of generated images and of a fixed real set, evaluated on the device.

    real       (N, 3, S, S) tiles: uint8, or float normalised to [-1, 1] (what the discriminator takes); kept where it is
               given (put it on the device once to keep evaluations free of uploads).
    n_fake     number of generated images (default len(real)).
    extractor  "discriminator": the labelled PROXY of fid.fid_proxy -- the discriminator trunk's features at native
               resolution, no resize; comparable only within one run, and the real statistics are recomputed at every call
               because the extractor moves with training.  A callable (fid.inception_features_device(weights)): images are
               resized to 299 x 299 first and the real statistics are computed once and cached.
    noise      None: (n_fake, E) standard normal values drawn ONCE from a private torch.Generator(seed) and reused at every
               evaluation (drawn at construction when ``encoding_dims`` is given, else at the first evaluation from the
               generator's ``encoding_dims`` -- the same values either way, the generator is private); a tensor: used as
               given; a callable noise(n): called at every evaluation.
    The metric never touches the global CPU or device random generators, puts both networks in eval mode under no_grad and
    restores their modes: a training run with the metric is bit-identical to one without it.
    Pickling (the trainer pickles its metrics into every checkpoint) keeps the settings only -- never the real set, the
    noise or cached statistics; an unpickled metric has to be given its data again (``set_real``) before it can evaluate."""

    def calculate_score(self, fake_stats, real_stats=None):
        (m1, s1), (m2, s2) = fake_stats[:2], real_stats[:2]
        from .fid import frechet_distance
        return frechet_distance(m1, s1, m2, s2)

    def metric_ops(self, generator, discriminator, device):
        from . import fid as FID
        fake, real = self._collect_sets(generator, discriminator, device, lambda batches, extract, resize: FID.device_statistics(
            batches, extract, resize=resize, value_range=(-1, 1)))
        return float(self.calculate_score(fake, real))


class KernelDistance(_GeneratedAgainstReal):
    """Kernel distance (KID, rna_gan_amd.kid) between features of generated images and of a fixed real set: the unbiased
    estimate of MMD^2 under the polynomial kernel (gamma <a, b> + coef0)^degree, gamma=None meaning 1 / F.  The Gram sums run on
    the device in fp64 (rg_polykernel_tile_sums); no covariance, no matrix square root.

    ``real``, ``n_fake``, ``extractor``, ``noise``, ``seed``, ``batch_size``, ``encoding_dims``: as FrechetDistance, with the
    same guarantees -- private noise, the global generators untouched, eval mode under no_grad with the modes restored, settings
    only in a pickle, ``set_real``.  The real set's FEATURES are cached only for a fixed (callable) extractor.
    num_subsets > 0: besides the full-set estimate, the estimate on ``num_subsets`` row subsets of ``subset_size`` rows (clamped
    to the smaller set) drawn without replacement from a private torch.Generator(seed) -- the same subsets at every evaluation;
    the published convention is 100 subsets of 1000.
    ``metric_ops`` returns the full-set ``mmd2``, or ``subset_mean`` when subsets are used: lower is better, about 0 when the
    two sets follow one distribution, and it can be slightly negative (the estimator is unbiased).  The whole dictionary of
    kid.kernel_distance is kept in ``self.last``."""

    SETTINGS, DROPPED = ("num_subsets", "subset_size", "degree", "gamma", "coef0"), ("last",)

    def __init__(self, real, n_fake=None, extractor="discriminator", noise=None, seed=0, batch_size=256, encoding_dims=None,
                 num_subsets=0, subset_size=1000, degree=3, gamma=None, coef0=1.0):
        super().__init__(real, n_fake, extractor, noise, seed, batch_size, encoding_dims)
        self.num_subsets, self.subset_size, self.degree = int(num_subsets), int(subset_size), int(degree)
        self.gamma, self.coef0 = (None if gamma is None else float(gamma)), float(coef0)
        if self.num_subsets < 0:
            raise ValueError("num_subsets must be >= 0")
        if self.subset_size < 2:
            raise ValueError("subset_size must be >= 2")
        if self.degree not in (1, 2, 3):
            raise ValueError("degree must be 1, 2 or 3")
        if self.gamma is not None and not self.gamma > 0.0:
            raise ValueError("gamma must be > 0 (or None for 1 / F)")
        self.last = None

    def calculate_score(self, fake_feats, real_feats=None):
        from .kid import kernel_distance
        return kernel_distance(fake_feats, real_feats, num_subsets=self.num_subsets, subset_size=self.subset_size, seed=self.seed,
                               gamma=self.gamma, coef0=self.coef0, degree=self.degree)

    def metric_ops(self, generator, discriminator, device):
        from . import fid as FID
        fake, real = self._collect_sets(generator, discriminator, device, lambda batches, extract, resize: FID.device_features(
            batches, extract, resize=resize, value_range=(-1, 1)))
        return self._record(self.calculate_score(fake, real), "subset_mean" if self.num_subsets > 0 else "mmd2")


class PrecisionRecall(_GeneratedAgainstReal):
    """Improved precision and recall (Kynkaanniemi et al. 2019) and density and coverage (Naeem et al. 2020) between features of
    generated images and of a fixed real set (rna_gan_amd.prdc): both manifolds are estimated by the k-nearest-neighbour balls of
    their rows.  precision / density fall when generated tiles leave the real manifold (low fidelity); recall / coverage fall
    when the generator produces only a few of the real patterns (mode collapse) -- which a single distance cannot tell apart.
    Radii and memberships run on the device in fp64 (rg_knn_radii2, rg_radius_hits), comparisons are ``<=`` on squared distances.

    ``real``, ``n_fake``, ``extractor``, ``noise``, ``seed``, ``batch_size``, ``encoding_dims``: as FrechetDistance, with the
    same guarantees -- private noise, the global generators untouched, eval mode under no_grad with the modes restored, ``set_real``.
    nearest_k  the neighbourhood size k, 1..16; both sets need at least k + 1 rows.
    report     which of "precision", "recall", "density", "coverage" ``metric_ops`` returns (what the trainer logs: one float
               per epoch).  The whole dictionary of the evaluation is kept in ``self.last`` and appended to ``self.history``.
    Pickling keeps the settings AND ``history`` (four floats per epoch, so a checkpoint holds all four values of every epoch),
    never the real set, the noise or cached features.  For a fixed (callable) extractor the real set's features and its radii
    are computed once and cached."""

    REPORTS = ("precision", "recall", "density", "coverage")
    SETTINGS, DROPPED, HISTORY = ("nearest_k", "report"), ("last", "_real_radii"), True

    def __init__(self, real, n_fake=None, extractor="discriminator", noise=None, seed=0, batch_size=256, encoding_dims=None,
                 nearest_k=5, report="recall"):
        self.nearest_k = int(nearest_k)
        if not 1 <= self.nearest_k <= 16:
            raise ValueError("nearest_k must be in 1..16")
        if report not in self.REPORTS:
            raise ValueError("report must be one of %s" % ", ".join(self.REPORTS))
        self.report = report
        self.last, self.history = None, []
        self._real_radii = None
        super().__init__(real, n_fake, extractor, noise, seed, batch_size, encoding_dims)
        if self.n_fake < self.nearest_k + 1:
            raise ValueError("n_fake is %d: nearest_k = %d needs at least %d generated images" % (self.n_fake, self.nearest_k, self.nearest_k + 1))

    def set_real(self, real):
        super().set_real(real)
        if self.real.shape[0] < self.nearest_k + 1:
            raise ValueError("real has %d tiles: nearest_k = %d needs at least %d" % (self.real.shape[0], self.nearest_k, self.nearest_k + 1))
        self._real_radii = None

    def calculate_score(self, fake_feats, real_feats=None, real_radii2=None):
        from .prdc import prdc
        return prdc(real_feats, fake_feats, k=self.nearest_k, real_radii2=real_radii2)

    def metric_ops(self, generator, discriminator, device):
        from . import fid as FID
        from .prdc import knn_radii2
        fake, real = self._collect_sets(generator, discriminator, device, lambda batches, extract, resize: FID.device_features(
            batches, extract, resize=resize, value_range=(-1, 1)))
        # a fixed extractor: the real features are cached, so are their radii
        radii = self._real_side("_real_radii", lambda: knn_radii2(real, self.nearest_k), self._real_stats is not None)
        return self._record(self.calculate_score(fake, real, radii), self.report)


class TissueYield(_GeneratedSamples):
    """The fraction of generated tiles that the reference tiler's acceptance rule keeps (rna_gan_amd.tissue.accept: the dilated
    tissue mask covers more than ``min_tissue`` of the tile and the tile is not low-contrast) -- the rule every real training tile
    passed and no generated tile is otherwise held to.  No real set and no feature extractor: ``samples`` generated images go
    through ``synthesize`` -> ``export.tiles_u8`` (the bytes a tile store would hold) -> ``tissue.tile_stats`` on the device; twelve
    integers per tile reach the host.

    noise, seed, batch_size, encoding_dims: as FrechetDistance -- (samples, E) standard normal values drawn once from a private
    torch.Generator(seed), a tensor, or a callable noise(n); the global generators are never touched, the generator runs in eval
    mode under no_grad and its mode is restored.  rgb_min, dilate, percentiles: of ``tile_stats``; fraction, luma_range: of
    ``low_contrast``.
    ``metric_ops`` returns the accepted fraction (what the trainer logs).  ``self.last`` and, per evaluation, ``self.history`` keep
    {"accepted", "tissue_fraction" (the mean over the tiles), "low_contrast" (the fraction of low-contrast tiles)}; the
    TileStats of the last evaluation is ``self.last_stats``.  Pickling keeps the settings and ``history``, never the noise."""

    SETTINGS = ("min_tissue", "fraction", "luma_range", "rgb_min", "dilate", "percentiles")
    DROPPED, HISTORY = ("last", "last_stats"), True

    def __init__(self, samples, min_tissue=0.2, rgb_min=50, dilate=3, percentiles=(1, 99), fraction=0.05, luma_range=2.0,
                 noise=None, seed=0, batch_size=256, encoding_dims=None):
        super().__init__(samples, noise, seed, batch_size, encoding_dims, count="samples")
        self.min_tissue, self.fraction, self.luma_range = float(min_tissue), float(fraction), float(luma_range)
        self.rgb_min, self.dilate, self.percentiles = int(rgb_min), int(dilate), tuple(float(q) for q in percentiles)
        from .tissue import MAX_DILATE, percentile_ranks
        if not 0 <= self.rgb_min <= 255 or not 0 <= self.dilate <= MAX_DILATE:
            raise ValueError("rgb_min must be in 0..255 and dilate in 0..%d" % MAX_DILATE)
        percentile_ranks(2, self.percentiles)                    # two percentiles in [0, 100]
        self.last, self.last_stats, self.history = None, None, []

    def calculate_score(self, stats):
        from . import tissue as TQ
        n = max(len(stats), 1)
        return {"accepted": float(TQ.accept(stats, self.min_tissue, self.fraction, self.luma_range).sum()) / n,
                "tissue_fraction": float(TQ.tissue_fraction(stats).sum()) / n,
                "low_contrast": float(TQ.low_contrast(stats, self.fraction, self.luma_range).sum()) / n}

    def metric_ops(self, generator, device):
        import numpy as np
        from . import tissue as TQ
        rows, H, W = [], 1, 1
        for tiles in self.generated_tiles(generator, device):
            H, W = int(tiles.shape[1]), int(tiles.shape[2])
            rows.append(TQ.tile_stats_device(tiles, rgb_min=self.rgb_min, dilate=self.dilate, percentiles=self.percentiles)[0])
        stats = TQ.stats_from_rows(torch.cat(rows).cpu().numpy() if rows else np.zeros((0, 12), np.int32), H, W, self.rgb_min,
                                   self.dilate, self.percentiles)                       # ONE download: 48 bytes per tile
        self.last_stats = stats
        return self._record(self.calculate_score(stats), "accepted")


class ConditioningFidelity(EvaluationMetric):
    """Does the generator follow the expression row it is conditioned on?  Per patient, the mean features of its real tiles and of
    ``tiles_per_patient`` tiles generated from its row (rna_gan_amd.representation: rg_group_sums_update on the device); every
    generated centroid then ranks its own patient's real centroid among all P real centroids (rg_match_ranks).  A generator that
    ignores its conditioning scores ``chance_top1`` = 1 / P whatever its tiles look like -- which FrechetDistance,
    KernelDistance, PrecisionRecall and TissueYield, all pooling the generated set into one cloud, cannot tell.

    real_tiles  (M, 3, S, S) tiles, uint8 or float normalised to [-1, 1]; kept where they are given.
    patient_of  (M,) integers: tile m belongs to patient patient_of[m]; every patient needs at least one tile.
    rna         (P >= 2, features) prepared expression rows, one per patient.
    betavae     the frozen encoder of the ``wganvae`` losses (run in eval mode, its mode restored).
    ``from_tile_set(ts, betavae, ...)`` takes the three tensors from a ``resident.DeviceTileSet`` with RNA.
    tiles_per_patient  generated tiles per patient; the noise is ``representation.conditioned_noise(seed, group)``: a private
                torch.Generator, the same values at every evaluation, the global generators never touched.
    extractor   "discriminator" (the labelled proxy: the critic's trunk at native resolution; the real centroids are recomputed
                at every call because the extractor moves with training) or a callable device-side extractor (images resized to
                299 x 299 first; the real centroids are computed once and cached).
    center      subtract each set's own grand mean before the distances (representation.match_ranks: the domain gap between
                generated and real features is a common offset that would otherwise decide every rank).
    report      which of "top1", "top5", "mrr", "median_rank" ``metric_ops`` returns; all scores of an evaluation are kept in
                ``self.last`` and appended to ``self.history``, the ranks in ``self.last_rank``.
    Both networks run in eval mode under no_grad and their modes are restored: a training run with the metric is bit-identical to
    one without it.  Pickling keeps the settings and ``history`` only; ``set_data`` re-supplies tiles, ids, rows and encoder."""

    REPORTS = ("top1", "top5", "mrr", "median_rank")
    SETTINGS = ("tiles_per_patient", "seed", "batch_size", "group", "center", "report", "extractor")
    DROPPED, HISTORY = ("real_tiles", "patient_of", "rna", "betavae", "_real_centroids", "last", "last_rank"), True

    def __init__(self, real_tiles, patient_of, rna, betavae, tiles_per_patient=8, extractor="discriminator", seed=0,
                 batch_size=256, center=True, report="top1", group=4096):
        super().__init__()
        self.extractor = _checked_extractor(extractor)
        if report not in self.REPORTS:
            raise ValueError("report must be one of %s" % ", ".join(self.REPORTS))
        self.report, self.center = report, bool(center)
        self.tiles_per_patient, self.seed, self.batch_size, self.group = int(tiles_per_patient), int(seed), int(batch_size), int(group)
        if self.tiles_per_patient < 1 or self.batch_size < 1 or self.group < 2:
            raise ValueError("tiles_per_patient and batch_size must be >= 1 and group >= 2")
        self.last, self.last_rank, self.history = None, None, []
        self.set_data(real_tiles, patient_of, rna, betavae)

    @classmethod
    def from_tile_set(cls, ts, betavae, **kwargs):
        if ts.rna is None:
            raise ValueError("ConditioningFidelity needs a tile set with RNA rows")
        return cls(ts.tiles, ts.row_of, ts.rna, betavae, **kwargs)

    def set_data(self, real_tiles, patient_of, rna, betavae):
        _checked_tiles(real_tiles, "real_tiles", "M", 0)
        if not torch.is_tensor(rna) or rna.dim() != 2 or rna.shape[0] < 2:
            raise ValueError("rna must be (P >= 2, features): a rank among fewer than two patients says nothing")
        patient_of = torch.as_tensor(patient_of)
        P = int(rna.shape[0])
        if patient_of.dim() != 1 or patient_of.shape[0] != real_tiles.shape[0] or patient_of.is_floating_point():
            raise ValueError("patient_of must hold one integer per tile")
        ids = patient_of.detach().cpu().long()
        if ids.numel() == 0 or int(ids.min()) < 0 or int(ids.max()) >= P:
            raise ValueError("patient_of points outside the %d rows of rna" % P)
        if int((torch.bincount(ids, minlength=P) == 0).sum()):
            raise ValueError("every patient needs at least one real tile")
        self.real_tiles, self.patient_of, self.rna, self.betavae = real_tiles, patient_of.to(torch.int32), rna, betavae
        self._real_centroids = None

    def calculate_score(self, fake_centroids, real_centroids=None):
        from .representation import match_ranks, retrieval_scores
        rank, _ = match_ranks(fake_centroids, real_centroids, None, self.center)
        self.last_rank = rank
        return retrieval_scores(rank, real_centroids.shape[0])

    @torch.no_grad()
    def metric_ops(self, generator, discriminator, device):
        self._require(self.real_tiles, "data", "set_data")
        from .representation import patient_representations
        with _eval_mode(generator, discriminator):
            extract, resize = feature_extractor(self.extractor, discriminator)
            have = self._real_centroids is not None
            reps = patient_representations(extract, real=None if have else (self.real_tiles, self.patient_of),
                                           conditioned=generator, betavae=self.betavae, gene_exp=self.rna,
                                           tiles_per_patient=self.tiles_per_patient, n_patients=self.rna.shape[0], seed=self.seed,
                                           batch_size=self.batch_size, group=self.group, resize=resize)
            real = self._real_side("_real_centroids", lambda: reps["real"], resize is not None)
            return self._record(self.calculate_score(reps["conditioned"], real), self.report)


class Memorisation(_GeneratedSamples):
    """Is the generator reproducing its training tiles?  The one failure every metric above REWARDS: a memorised tile is perfect in
    fidelity, covers its real neighbour and follows its patient's expression row.  ``samples`` generated tiles go through
    ``synthesize`` -> ``export.tiles_u8(layout="nchw")`` and are searched against the int8 block-mean descriptors of the training
    tiles (rna_gan_amd.nearest: rg_tile_descriptor_i8, rg_nn_topk_i8 on the integer matrix cores -- exact integers); a sample counts
    as copied when it is closer to its nearest training tile than any OTHER training tile is (Alaa et al. 2022).  Samples of the
    training distribution itself are flagged about half of the time, so ``copy_rate`` near 0.5 is what a generator that does not
    memorise converges to; copying pushes it towards 1 (nearest.audit).

    train_tiles  (M, C, S, S) uint8 tiles, kept where they are given (``from_tile_set(ts, ...)``: a resident.DeviceTileSet's), or
                 None until ``set_train``.  The descriptor index is built on first use and kept.
    factor       the descriptor's block size (nearest.FACTORS);  k: neighbours kept per sample (``self.last_result``).
    d4           search every sample under all eight symmetries of the square (training under augment="d4").
    heldout      real uint8 tiles the generator never saw: adds ``closer_than_heldout`` (Meehan et al. 2020).
    noise, seed, batch_size, encoding_dims: as TissueYield; the generator runs in eval mode under no_grad, its mode is restored.
    ``metric_ops`` returns ``copy_rate`` (what the trainer logs); ``self.last`` and, per evaluation, ``self.history`` keep
    {"copy_rate", "exact", "min_d2", "median_d2"} and "closer_than_heldout" when held-out tiles were given.  An exact duplicate pair
    inside the training set has loo_d2 = 0: a copy of either is never ``copied`` and shows in "exact" (nearest.audit).
    Data parallel: the metric audits against the tiles it was given -- with ``from_tile_set`` the RANK'S OWN SHARD, as
    ConditioningFidelity.from_tile_set does; there is no index across ranks, so a copy of another rank's tile is not seen.
    Pickling keeps the settings and ``history``; tiles, index and noise are never pickled (``set_train`` re-supplies the tiles)."""

    SETTINGS, DROPPED, HISTORY = ("factor", "k", "d4"), ("train_tiles", "heldout", "_index", "last", "last_result"), True
    LAYOUT = "nchw"                # planar uint8 tiles: the training set's layout

    def __init__(self, train_tiles, samples, factor=4, k=1, d4=False, heldout=None, noise=None, seed=0, batch_size=256,
                 encoding_dims=None):
        super().__init__(samples, noise, seed, batch_size, encoding_dims, count="samples")
        from .nearest import FACTORS, K_MAX
        self.factor, self.k, self.d4 = int(factor), int(k), bool(d4)
        if self.factor not in FACTORS or not 1 <= self.k <= K_MAX:
            raise ValueError("factor must be one of %s and k in 1..%d" % (FACTORS, K_MAX))
        self.last, self.last_result, self.history = None, None, []
        self.train_tiles = self.heldout = self._index = None
        self.set_train(train_tiles, heldout)

    @classmethod
    def from_tile_set(cls, ts, samples, **kwargs):
        return cls(ts.tiles, samples, **kwargs)

    def set_train(self, train_tiles, heldout=None):
        train_tiles = getattr(train_tiles, "tiles", train_tiles)
        for t in (train_tiles, heldout):
            if t is not None and (not torch.is_tensor(t) or t.dtype != torch.uint8 or t.dim() != 4):
                raise ValueError("training and held-out tiles are (M, C, S, S) uint8 tensors")
        self.train_tiles, self.heldout, self._index = train_tiles, heldout, None

    def calculate_score(self, generated_u8):
        from .nearest import TrainIndex, audit
        if self._index is None:
            self._index = TrainIndex(self.train_tiles, factor=self.factor)
        heldout = None if self.heldout is None else self.heldout.to(self._index.device)
        self.last_result = audit(generated_u8.to(self._index.device), self._index, k=self.k, d4=self.d4, heldout_u8=heldout)
        return self.last_result.summary()

    def metric_ops(self, generator, device):
        self._require(self.train_tiles, "training tiles", "set_train")
        return self._record(self.calculate_score(torch.cat(self.generated_tiles(generator, device))), "copy_rate")


class PairDiversity(_GeneratedSamples):
    """Are the generated tiles different from each other?  The mean MS-SSIM over ``pairs`` fixed random pairs of ``samples`` generated
    tiles (Odena et al. 2017; rna_gan_amd.msssim: rg_msssim_pyramid, rg_msssim_pairs) -- the pixel-space sign of mode collapse that
    needs no feature extractor: a collapsing generator keeps its tissue yield, copies nothing and moves the critic-feature distances
    only slowly, while its tiles grow alike.  ``samples`` generated images go through ``synthesize`` -> ``export.tiles_u8`` (the bytes
    a tile store would hold) -> the pair launch; P * S * 6 doubles reach the host.

    pairs     how many pairs (default: ``samples``); the list is ``msssim.random_pairs(samples, pairs, seed)``, the same at every
              evaluation, and never pairs a tile with itself.
    real      None, or real uint8 tiles -- (N, 3, H, W) or (N, H, W, 3), or a resident.DeviceTileSet -- of the generated tiles' size,
              N >= samples: the SAME pair list is evaluated over them once, at the first evaluation, and cached.  Generated pairs
              clearly more similar than real pairs (a positive ``gap``) mean collapse.
    scales    S of ``msssim.components`` (default: the largest the tile size allows).
    noise, seed, batch_size, encoding_dims: as TissueYield; the generator runs in eval mode under no_grad, its mode is restored.
    ``metric_ops`` returns the mean MS-SSIM of the generated pairs (what the trainer logs); ``self.last`` and, per evaluation,
    ``self.history`` keep {"generated", "real", "gap" (generated - real; both None without real tiles), "per_scale" ([S][2]: the means
    of CS_s and SSIM_s over the generated pairs)}; the per-pair scores of the last evaluation are ``self.last_scores``.
    Pickling keeps the settings and ``history``, never the noise or the tiles (``set_real`` re-supplies the real tiles)."""

    SETTINGS, DROPPED, HISTORY = ("pairs", "scales"), ("real", "_real_score", "last", "last_scores"), True

    def __init__(self, samples, pairs=None, real=None, scales=None, noise=None, seed=0, batch_size=256, encoding_dims=None):
        super().__init__(samples, noise, seed, batch_size, encoding_dims, count="samples", least=2)
        self.pairs = self.n_fake if pairs is None else int(pairs)
        if self.pairs < 1:
            raise ValueError("pairs must be >= 1")
        self.scales = None if scales is None else int(scales)
        if self.scales is not None and not 1 <= self.scales <= 5:
            raise ValueError("scales must be in 1..5")
        self.last, self.last_scores, self.history = None, None, []
        self.real = self._real_score = None
        self.set_real(real)

    def set_real(self, real):
        tiles = getattr(real, "tiles", real)
        if tiles is not None:
            if not torch.is_tensor(tiles) or tiles.dtype != torch.uint8 or tiles.dim() != 4 or 3 not in (tiles.shape[1], tiles.shape[3]):
                raise ValueError("real must be uint8 tiles, (N, 3, H, W) or (N, H, W, 3), or a DeviceTileSet")
            if tiles.shape[0] < self.n_fake:
                raise ValueError("real holds %d tiles, the pair list runs over %d" % (tiles.shape[0], self.n_fake))
        self.real, self._real_score = tiles, None

    def pair_list(self):
        from .msssim import random_pairs
        return random_pairs(self.n_fake, self.pairs, self.seed)

    def calculate_score(self, tiles, layout="nhwc"):
        """(the per-pair MS-SSIM, the diversity dictionary) of the metric's pair list over a tile set"""
        from . import msssim as MS
        comp = MS.components(tiles, None, self.pair_list(), self.scales, layout)
        return MS.finish(comp), MS.diversity_of(comp)

    def metric_ops(self, generator, device):
        tiles = torch.cat(self.generated_tiles(generator, device))
        self.last_scores, gen = self.calculate_score(tiles)
        def real_mean():
            if self.real is None:
                return None
            real = self.real.to(device)
            return self.calculate_score(real, "nchw" if real.shape[1] == 3 else "nhwc")[1]["mean"]
        real = self._real_side("_real_score", real_mean, True)       # pixel space: the real tiles' score never changes
        return self._record({"generated": gen["mean"], "real": real, "gap": None if real is None else gen["mean"] - real,
                             "per_scale": gen["per_scale"]}, "generated")
