"""Per-patient representations and the retrieval that turns them into a conditioning score, evaluated on the device.

Counterpart of src/compute_representation.py: per patient, the mean feature vector of its real tiles, of tiles generated from its
expression row, and of unconditioned tiles.  The reference downloads every activation and averages with numpy; here the features
stay on the device and are reduced PER GROUP by rg_group_sums_update (include/rnagan_hip.h): one fp64 chain of additions per
(patient, feature) in row order, no floating-point atomics -- the same bits on every run and for every batching of the rows, which
``index_add_`` does not give.  Only the (P, F) centroids are ever downloaded.

What the reference does not do is ask the question the centroids answer: do the tiles generated from patient p's expression row
look like patient p?  ``match_ranks`` ranks, for every generated centroid, its own patient's real centroid among all real
centroids by squared distance (rg_match_ranks: fp64, ties broken by index), and ``retrieval_scores`` summarises the ranks: a
generator that ignores its conditioning scores ``chance_top1``, one that honours it scores towards 1.

Centring.  Generated and real features differ by a domain gap that is, to first order, one common offset.  Left in, the offset is
part of every distance, and every generated centroid ranks first the real centroids that lie along the gap, whoever they belong
to.  ``match_ranks(center=True)`` therefore subtracts from each set ITS OWN grand mean (fp64, in torch) before the distances:
what is compared is where a patient lies within its set.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _abi
from .kid import _row_pair, _rows


class GroupMeans:
    """Running per-group sums of (n, F) fp32 feature rows, kept on the device in fp64 by rg_group_sums_update: sums (G, F) fp64
    and counts (G,) int64.  The sum of an entry is ONE chain of additions in the order the rows were handed over, whatever the
    batching."""

    def __init__(self, G, F, device):
        self.G, self.F = int(G), int(F)
        if self.G < 1 or self.F < 1:
            raise ValueError("GroupMeans: G and F must be >= 1")
        self.device = torch.device(device)
        self.sums = torch.zeros(self.G, self.F, dtype=torch.float64, device=self.device)
        self._counts = torch.zeros(self.G, dtype=torch.int64, device=self.device)
        self.n = 0

    def update(self, feats, group):
        """feats (n, F) fp32 on the device (unit column stride, row stride >= F is read in place; any other form is copied once);
        group (n,) int32 ids on the device: rows with an id outside [0, G) are ignored."""
        feats, ldx = _rows(feats, "GroupMeans.update: feats")
        if feats.shape[1] != self.F or feats.device != self.sums.device:
            raise ValueError("GroupMeans.update: expected (n, %d) on %s, got %s on %s"
                             % (self.F, self.sums.device, tuple(feats.shape), feats.device))
        n = feats.shape[0]
        if not (torch.is_tensor(group) and group.dtype == torch.int32 and group.device == feats.device and tuple(group.shape) == (n,)):
            raise TypeError("GroupMeans.update takes the group ids as an (n,) int32 tensor on the features' device")
        group = group.contiguous()
        _abi.launch("rg_group_sums_update", self.sums.device, feats.data_ptr(), ldx, n, self.F, group.data_ptr(), self.G,
                    self.sums.data_ptr(), self._counts.data_ptr())
        self.n += n
        return self

    def counts(self):
        """(G,) int64 device tensor: the rows counted per group so far"""
        return self._counts.clone()

    def means(self):
        """(G, F) fp64 on the device: sums / counts, one IEEE division per entry.  Raises for a group without rows."""
        empty = torch.nonzero(self._counts == 0).flatten().tolist()
        if empty:
            raise ValueError("GroupMeans.means: %d group(s) have no rows (the first: %d)" % (len(empty), empty[0]))
        return self.sums / self._counts.to(torch.float64)[:, None]


def group_means(batches_with_ids, extractor, G, resize=None, value_range=None):
    """fid.device_features' loop and checks over an iterable of (device image batch, (n,) int32 device ids), feeding a
    GroupMeans: the features never leave the device and are never concatenated.  Returns the GroupMeans."""
    from .fid import preprocess_images_device
    acc = None
    for batch, ids in batches_with_ids:
        if resize is not None:
            batch = preprocess_images_device(batch, resize, value_range)
        f = extractor(batch)
        if not (torch.is_tensor(f) and f.is_cuda):
            raise TypeError("group_means needs an extractor that returns device tensors (discriminator_features_device, "
                            "inception_features_device)")
        if f.dim() != 2 or f.shape[0] != ids.shape[0] or (acc is not None and (f.shape[1] != acc.F or f.device != acc.device)):
            raise ValueError("group_means: the extractor returned %s for %d ids%s" % (
                tuple(f.shape), ids.shape[0], "" if acc is None else " after (n, %d)" % acc.F))
        if acc is None:
            acc = GroupMeans(G, f.shape[1], f.device)
        acc.update(f.float(), ids)
    if acc is None:
        raise ValueError("group_means: no batches")
    return acc


def match_ranks(query, ref, target=None, center=True):
    """``(rank int32, dtarget fp64)``, device tensors of len(query): for every row r of ``query`` (Pq, F) the rank of row
    target[r] of ``ref`` (Pr, F) among all rows of ref by squared distance to query[r] -- 0 = the designated partner is the
    nearest row, ties broken by index -- and that squared distance (rg_match_ranks).  Both sets are fp64 on one device.
    target: None (row r's partner is row r; needs Pq <= Pr) or Pq integers in [0, Pr).
    center=True: each set's own grand mean is subtracted first (see the module docstring)."""
    # (P, 0) centroids have always been refused as a TypeError here
    query, lda, ref, ldb = _row_pair(query, ref, ("query", "ref"), torch.float64, no_columns=TypeError)
    na, nb, F = query.shape[0], ref.shape[0], query.shape[1]
    if na < 1 or nb < 1:
        raise ValueError("match_ranks needs at least one row in each set, got %d and %d" % (na, nb))
    if target is None:
        if na > nb:
            raise ValueError("match_ranks without target needs len(query) <= len(ref), got %d and %d" % (na, nb))
    else:
        target = torch.as_tensor(target)
        if target.dim() != 1 or target.shape[0] != na or target.is_floating_point():
            raise ValueError("target must be %d integers" % na)
        if not (0 <= int(target.min()) and int(target.max()) < nb):       # the kernel's clamp is never relied upon
            raise ValueError("target points outside ref")
        target = target.to(device=query.device, dtype=torch.int32).contiguous()
    if center:
        query, ref = (query - query.mean(dim=0, keepdim=True)).contiguous(), (ref - ref.mean(dim=0, keepdim=True)).contiguous()
        lda = ldb = F
    rank = torch.empty(na, dtype=torch.int32, device=query.device)
    dtarget = torch.empty(na, dtype=torch.float64, device=query.device)
    _abi.launch("rg_match_ranks", query.device, query.data_ptr(), lda, na, ref.data_ptr(), ldb, nb, F,
                None if target is None else target.data_ptr(), rank.data_ptr(), dtarget.data_ptr())
    return rank, dtarget


def retrieval_scores(rank, n_ref):
    """{"top1", "top5", "mrr", "median_rank", "chance_top1"} (Python floats) of the ranks of match_ranks against ``n_ref``
    reference rows, computed on the host from the downloaded integers: top1 = mean(rank == 0), top5 = mean(rank < min(5, n_ref)),
    mrr = mean(1 / (rank + 1)), chance_top1 = 1 / n_ref."""
    r = rank.detach().cpu().numpy() if torch.is_tensor(rank) else np.asarray(rank)
    r = r.astype(np.int64)
    n_ref = int(n_ref)
    if r.ndim != 1 or r.size < 1 or n_ref < 1:
        raise ValueError("retrieval_scores takes at least one rank and n_ref >= 1")
    return {"top1": float(np.mean(r == 0)), "top5": float(np.mean(r < min(5, n_ref))), "mrr": float(np.mean(1.0 / (r + 1.0))),
            "median_rank": float(np.median(r)), "chance_top1": 1.0 / n_ref}


def latent_prep(u, z):
    """u + z standardised per column over the rows handed in (rg_latent_prep), u and z contiguous (n, E) fp32 on one device:
    the rank-local form, no collective (HipOps.latent_prep has the one with synchronised statistics)"""
    out = torch.empty_like(u)
    _abi.launch("rg_latent_prep", u.device, u.data_ptr(), z.data_ptr(), out.data_ptr(), u.shape[0], u.shape[1])
    return out


def conditioned_noise(generator, betavae, gene_exp, tiles_per_patient, seed, group=4096):
    """The conditioned noise of ``gan_utils.generate_tiles``, group by group: a generator function over
    ``(patient_index, noise)`` -- (n,) int32 and (n, E) fp32 device tensors -- for ``tiles_per_patient`` tiles of each of the P
    prepared expression rows of ``gene_exp``, on the generator's device.

    * The frozen encoder runs ONCE over the P rows, in eval mode (its mode is restored).
    * The uniform draw U(-0.3, 0.3) comes from a PRIVATE ``torch.Generator`` seeded with ``seed``.
    * The request is walked tile-major (tile index outer, patient inner) in groups of at most ``group`` rows; each group is ONE
      ``latent_prep(u, z)`` call (the column standardisation over the group); a trailing group of fewer than 2 rows joins the
      previous one (``gan_utils._tile_groups``)."""
    from .gan_utils import _tile_groups
    if gene_exp.dim() != 2 or gene_exp.shape[0] < 1:
        raise ValueError("gene_exp must be (P, features) with P >= 1")
    P, T, group = gene_exp.shape[0], int(tiles_per_patient), int(group)
    total = P * T
    if T < 1 or total < 2:
        raise ValueError("conditioned noise needs at least 2 tiles in all (the column standardisation divides by n - 1)")
    if group < 2:
        raise ValueError("group must be at least 2")
    device = next(generator.parameters()).device
    prep = generator.runtime()[0].latent_prep if hasattr(generator, "runtime") else latent_prep
    betavae = betavae.to(device)
    was_training = betavae.training
    betavae.eval()
    try:
        with torch.no_grad():
            z = betavae.encode(gene_exp.to(device))[0].detach().float().contiguous()
    finally:
        betavae.train(was_training)
    private = torch.Generator().manual_seed(int(seed))
    for r0, r1 in _tile_groups(total, group):
        patient = (torch.arange(r0, r1) % P).to(device)
        u = torch.empty(r1 - r0, generator.encoding_dims).uniform_(-0.3, 0.3, generator=private).to(device)
        with torch.no_grad():
            noise = prep(u.contiguous(), z[patient].contiguous())
        yield patient.to(torch.int32), noise


def _real_batch(x, resize, mean, std):
    """a chunk of real tiles in the form its consumer takes: uint8 as it is for the resize kernel; for an extractor at native
    resolution, uint8 tiles normalised by the training input transform (rg_u8_to_norm)"""
    if resize is not None or x.dtype != torch.uint8:
        return x if x.dtype == torch.uint8 else x.float()
    x = x.contiguous()
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    _abi.launch("rg_u8_to_norm", x.device, x.data_ptr(), y.data_ptr(), x.numel(), float(mean), float(std))
    return y


def _generated(generator, noise, batch_size):
    from .gan_utils import synthesize
    from .models import DCGANGenerator
    for c in torch.split(noise, batch_size):
        if isinstance(generator, DCGANGenerator):
            yield synthesize(generator, c, chunk=batch_size)
        else:
            yield generator(c.contiguous())


@torch.no_grad()
def real_representations(real, extractor, n_patients=None, resize=None, batch_size=256, mean=0.5, std=0.5):
    """(P, F) fp64 device tensor: per patient, the mean features of its real tiles.  real: a ``resident.DeviceTileSet`` with RNA
    (patients = the rows of its de-duplicated table) or ``(tiles, patient_of)`` -- (M, 3, S, S) uint8 or [-1, 1] float tiles and
    (M,) integer patient ids; tiles that are not on the extractor's device yet are uploaded chunk by chunk."""
    if isinstance(real, (tuple, list)):
        tiles, patient_of = real
        patient_of = torch.as_tensor(patient_of)
        P = int(n_patients) if n_patients is not None else int(patient_of.max()) + 1
    else:
        if real.rna is None:
            raise ValueError("a DeviceTileSet without RNA rows has no patients")
        tiles, patient_of, P = real.tiles, real.row_of, int(real.rna.shape[0])
    if tiles.dim() != 4 or patient_of.shape[0] != tiles.shape[0] or tiles.shape[0] < 1:
        raise ValueError("real: one patient id per tile, at least one tile")
    device = tiles.device if tiles.is_cuda else torch.device("cuda", torch.cuda.current_device())
    patient_of = patient_of.to(device=device, dtype=torch.int32)

    def batches():
        for i in range(0, tiles.shape[0], batch_size):
            yield _real_batch(tiles[i:i + batch_size].to(device), resize, mean, std), patient_of[i:i + batch_size]
    value_range = None if tiles.dtype == torch.uint8 else (-1, 1)
    return group_means(batches(), extractor, P, resize=resize, value_range=value_range).means()


@torch.no_grad()
def patient_representations(extractor, real=None, conditioned=None, unconditioned=None, *, betavae=None, gene_exp=None,
                            tiles_per_patient=None, n_patients=None, seed=0, batch_size=256, group=4096, resize=None,
                            mean=0.5, std=0.5, noise=None):
    """The per-patient mean features of up to three sources, each a (P, F) fp64 device tensor under its key of the returned dict:

    "real"           ``real``: see ``real_representations``.
    "conditioned"    ``conditioned``: a generator conditioned on the P prepared expression rows ``gene_exp`` through ``betavae``:
                     ``tiles_per_patient`` tiles per patient from ``conditioned_noise(..., seed, group)``, synthesised by
                     ``gan_utils.synthesize`` (a ``DCGANGenerator``: eval-mode BatchNorm) or by a plain call of any other module.
    "unconditioned"  ``unconditioned``: a generator fed P * tiles_per_patient rows of standard normal noise from a private
                     ``torch.Generator(seed)`` (or the ``noise`` tensor given), rows dealt to the patients tile-major as the
                     conditioned ones are: what the centroids look like when nothing ties them to a patient.

    extractor: batch -> (n, F) fp32 device features; resize=299 puts ``fid.preprocess_images_device`` in front (an Inception
    extractor), resize=None hands the [-1, 1] images over at native resolution (``fid.discriminator_features_device``).
    The modules are used in the mode they are in; ``synthesize`` puts a DCGANGenerator in eval mode and restores it."""
    out = {}
    if real is not None:
        out["real"] = real_representations(real, extractor, n_patients, resize, batch_size, mean, std)
    T = None if tiles_per_patient is None else int(tiles_per_patient)
    if conditioned is not None:
        if betavae is None or gene_exp is None or T is None:
            raise ValueError("a conditioned generator needs betavae, gene_exp and tiles_per_patient")
        P = int(gene_exp.shape[0])

        def batches():
            for patient, z in conditioned_noise(conditioned, betavae, gene_exp, T, seed, group):
                pos = 0
                for img in _generated(conditioned, z.float(), batch_size):
                    yield img, patient[pos:pos + img.shape[0]]
                    pos += img.shape[0]
        out["conditioned"] = group_means(batches(), extractor, P, resize=resize, value_range=(-1, 1)).means()
    if unconditioned is not None:
        P = int(gene_exp.shape[0]) if gene_exp is not None else (int(n_patients) if n_patients is not None else None)
        if P is None or T is None:
            raise ValueError("an unconditioned generator needs tiles_per_patient and n_patients (or gene_exp)")
        device = next(unconditioned.parameters()).device
        if noise is None:
            noise = torch.randn(P * T, int(unconditioned.encoding_dims), generator=torch.Generator().manual_seed(int(seed)))
        if noise.shape[0] != P * T:
            raise ValueError("noise has %d rows, %d patients x %d tiles need %d" % (noise.shape[0], P, T, P * T))
        noise = noise.to(device).float()
        patient = (torch.arange(P * T) % P).to(device=device, dtype=torch.int32)

        def batches():
            pos = 0
            for img in _generated(unconditioned, noise, batch_size):
                yield img, patient[pos:pos + img.shape[0]]
                pos += img.shape[0]
        out["unconditioned"] = group_means(batches(), extractor, P, resize=resize, value_range=(-1, 1)).means()
    return out


def _feature_rows(batches_with_ids, extractor, resize=None, value_range=None):
    """group_means' loop and checks without the reduction: ``(feats (n, F) fp32, ids (n,) int32)``, device tensors, of an iterable
    of (device image batch, (n,) int32 device ids)"""
    from .fid import preprocess_images_device
    feats, rows = [], []
    for batch, ids in batches_with_ids:
        if resize is not None:
            batch = preprocess_images_device(batch, resize, value_range)
        f = extractor(batch)
        if not (torch.is_tensor(f) and f.is_cuda):
            raise TypeError("tile_features needs an extractor that returns device tensors (discriminator_features_device, "
                            "inception_features_device)")
        if f.dim() != 2 or f.shape[0] != ids.shape[0] or (feats and (f.shape[1] != feats[0].shape[1] or f.device != feats[0].device)):
            raise ValueError("tile_features: the extractor returned %s for %d ids%s" % (
                tuple(f.shape), ids.shape[0], " after (n, %d)" % feats[0].shape[1] if feats else ""))
        feats.append(f.float())
        rows.append(ids)
    if not feats:
        raise ValueError("tile_features: no batches")
    return torch.cat(feats).contiguous(), torch.cat(rows).contiguous()


@torch.no_grad()
def tile_features(extractor, real=None, conditioned=None, *, betavae=None, gene_exp=None, tiles_per_patient=None, seed=0,
                  batch_size=256, group=4096, resize=None, mean=0.5, std=0.5):
    """``patient_representations`` without the reduction: per source a pair ``(feats (n, F) fp32, row (n,) int32)`` of device
    tensors -- the features of every tile with the index of the patient (expression row) it belongs to -- for what needs the
    tiles themselves rather than centroids (rna_gan_amd.linprobe.tstr, tissue_probe.py).

    "real"         ``real = (tiles, patient_of)``: as ``real_representations`` takes it; the rows come back in tile order.
    "conditioned"  ``conditioned``: a generator; ``tiles_per_patient`` tiles per row of ``gene_exp`` from
                   ``conditioned_noise(..., seed, group)`` -- the SAME noise, so the same generated tiles, as the "conditioned"
                   source of ``patient_representations`` for the same seed -- in its tile-major order."""
    out = {}
    if real is not None:
        tiles, patient_of = real
        patient_of = torch.as_tensor(patient_of)
        if tiles.dim() != 4 or patient_of.shape[0] != tiles.shape[0] or tiles.shape[0] < 1:
            raise ValueError("real: one patient id per tile, at least one tile")
        device = tiles.device if tiles.is_cuda else torch.device("cuda", torch.cuda.current_device())
        patient_of = patient_of.to(device=device, dtype=torch.int32)

        def batches():
            for i in range(0, tiles.shape[0], batch_size):
                yield _real_batch(tiles[i:i + batch_size].to(device), resize, mean, std), patient_of[i:i + batch_size]
        out["real"] = _feature_rows(batches(), extractor, resize, None if tiles.dtype == torch.uint8 else (-1, 1))
    if conditioned is not None:
        if betavae is None or gene_exp is None or tiles_per_patient is None:
            raise ValueError("a conditioned generator needs betavae, gene_exp and tiles_per_patient")

        def batches():
            for patient, z in conditioned_noise(conditioned, betavae, gene_exp, int(tiles_per_patient), seed, group):
                pos = 0
                for img in _generated(conditioned, z.float(), batch_size):
                    yield img, patient[pos:pos + img.shape[0]]
                    pos += img.shape[0]
        out["conditioned"] = _feature_rows(batches(), extractor, resize, (-1, 1))
    return out
