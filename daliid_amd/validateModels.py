"""Mirror of the reference's ``validateModels.py`` for the path in scope (validateModels.py:26-76, 108-118):
``validationManager.getValidator(name)`` -> object with ``setParameters`` / ``validate(queries, gallery, model)`` /
``calculateMetrics``.  Feature normalisation + ``1 - q @ g.T`` run as ONE fused call on the MFMA distance kernel and
CMC/mAP on the GPU ranking kernel; the features never leave the device."""
import numpy as np
import torch

from .getFeatures import extractFeatures
from . import ops_eval


class validateModels:

    precision = "bf16x3"          # "bf16" trades ~1e-4 absolute distance error for ~2x distance throughput
    distmat_on_cpu = False        # the reference returns a CPU tensor (validateModels.py:58); 4 GB at config-5 size
    cam_label_of = view_label_of = None      # setSIE
    query_expansion = None        # setQueryExpansion
    report_minp = False           # True: calculateMetrics also computes mINP, prints it and leaves it in self.mINP

    def setParameters(self, img_height, img_width, rerank, gpu_index):
        self.img_height = img_height
        self.img_width = img_width
        self.rerank = rerank
        self.gpu_index = gpu_index

    def setSIE(self, cam_label_of=None, view_label_of=None):
        """For a model with SIE embeddings: callables from a subset (the rows handed to ``validate`` / ``validate_sharded`` / ``retrieve``) to the integer camera /
        view label of every row.  Without this call nothing changes."""
        self.cam_label_of, self.view_label_of = cam_label_of, view_label_of

    def setQueryExpansion(self, k=10, alpha=3.0, times=1, expand="all"):
        """Query expansion (expand="all": AQE / alpha-QE over [queries; gallery]) or database augmentation (expand="gallery") of the
        extracted features before ``distance`` in ``validate`` / ``retrieve`` / ``retrieve_features`` (ops_eval.query_expansion); with
        ``rerank`` the three blocks are computed from the expanded features.  ``setQueryExpansion(None)`` switches it off.  Without this
        call nothing changes."""
        if k is None:
            self.query_expansion = None
            return
        if expand not in ("all", "gallery"):
            raise ValueError("setQueryExpansion: expand must be 'all' or 'gallery', got %r" % (expand,))
        self.query_expansion = dict(k=k, alpha=alpha, times=times, expand=expand)

    def _expand(self, queries_fvs, gallery_fvs):
        if self.query_expansion is None:
            return queries_fvs, gallery_fvs
        return ops_eval.query_expansion(queries_fvs, gallery_fvs, precision=self.precision, **self.query_expansion)

    def _features(self, subset, model):
        side = {}
        if self.cam_label_of is not None:
            side["cam_labels"] = self.cam_label_of(subset)
        if self.view_label_of is not None:
            side["view_labels"] = self.view_label_of(subset)
        return extractFeatures(subset, self.img_height, self.img_width, model, 500, self.gpu_index, keep_on_device=True, **side)

    def validate(self, queries, gallery, model):
        model.eval()
        queries_fvs = self._features(queries, model)
        gallery_fvs = self._features(gallery, model)
        queries_fvs, gallery_fvs = self._expand(queries_fvs, gallery_fvs)
        distmat = self.distance(queries_fvs, gallery_fvs)
        if getattr(self, "rerank", False):
            # validateModels.py:49-53 (commented out in the reference): every block is the same cosine distance, so the three agree
            print('Applying person re-ranking ...')
            distmat_qq = self.distance(queries_fvs, queries_fvs)
            distmat_gg = self.distance(gallery_fvs, gallery_fvs)
            distmat = ops_eval.re_ranking(distmat, distmat_qq, distmat_gg)
            del distmat_qq, distmat_gg          # g_g is ng^2 floats (1 GB at Market size): gone before the ranking
        del queries_fvs, gallery_fvs
        cmc, mAP = self.calculateMetrics(distmat, queries, gallery)
        return cmc, mAP, (distmat.cpu() if self.distmat_on_cpu else distmat)

    def validate_sharded(self, queries, gallery, model, process_group=None):
        """``validate`` with the gallery split over the ranks of ``process_group`` (one process per GPU): every rank extracts
        the query features and the features of ITS contiguous gallery slice, computes its [Nq, Ng / N] block of ``1 - q @ g.T`` and the
        ranks merge per-query hit counts (ops_eval.rank_eval_sharded: one all-gather of match keys, one all-reduce of integer bins).
        -> (cmc, mAP, this rank's distance block); cmc / mAP are identical on every rank and, GIVEN the same model state on every rank,
        equal to the single-GPU result bit for bit.  The weights are identical by construction (parallel.py); the BatchNorm running
        statistics are rank-local during training and are made rank 0's at the end of every ``trainer.train`` epoch
        (parallel.sync_buffers_from_rank0, the nn.DataParallel semantics of Encoders.py:39-40).  A model whose statistics still differ
        between ranks is refused here, collectively, before any feature is extracted."""
        import torch.distributed as dist
        from . import _lib, parallel
        if getattr(self, "rerank", False):   # raised on every rank before any collective
            raise NotImplementedError("validate_sharded: re-ranking needs every gallery row's neighbourhood on one device; "
                                      "use validate() for rerank=True")
        if self.query_expansion is not None:   # likewise: on every rank, before any collective
            raise NotImplementedError("validate_sharded: query expansion needs every row's neighbours on one device; "
                                      "use validate(), or setQueryExpansion(None)")
        world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        rank = dist.get_rank(process_group) if dist.is_initialized() else 0
        model.eval()
        if not parallel.buffers_in_sync((model,), process_group):
            raise _lib.DaliError("validate_sharded: BatchNorm running statistics differ between ranks "
                                 "(call parallel.sync_buffers_from_rank0 or load the same checkpoint on every rank)")
        lo, hi = ops_eval.shard_bounds(len(gallery), world)[rank:rank + 2]
        queries_fvs = self._features(queries, model)
        if hi > lo:
            gallery_fvs = self._features(gallery[lo:hi], model)
        else:                  # trailing ranks of a small gallery hold no rows (128-row aligned slices): an empty block, same collectives
            gallery_fvs = queries_fvs.new_zeros(0, queries_fvs.shape[1])
        block = self.distance(queries_fvs, gallery_fvs)
        del queries_fvs, gallery_fvs
        cmc, mAP = ops_eval.rank_eval_sharded(block, queries[:, 1], gallery[lo:hi, 1], queries[:, 2], gallery[lo:hi, 2], lo, process_group,
                                              max_rank=50, ng_total=len(gallery))
        return cmc, mAP, block

    def distance(self, queries_fvs, gallery_fvs):
        """validateModels.py:41-47: q/|q|, g/|g|, 1 - q @ g.T (fused)."""
        return ops_eval.pairdist(queries_fvs.contiguous(), gallery_fvs.contiguous(), metric="cosine", precision=self.precision, normalize=True)

    def retrieve(self, queries, gallery, model, k=50):
        """The k nearest gallery images of every query under ``validate``'s distance, without the [Nq, Ng] matrix
        (ops_eval.pairdist_topk): -> (indices int32 [Nq, k] into ``gallery``, distances fp32 [Nq, k]) on the device, nearest first, exact
        ties by ascending gallery index.  The distances are bitwise the entries ``validate`` would return in its matrix."""
        model.eval()
        queries_fvs = self._features(queries, model)
        gallery_fvs = self._features(gallery, model)
        return self.retrieve_features(queries_fvs, gallery_fvs, k)

    def retrieve_features(self, queries_fvs, gallery_fvs, k=50):
        queries_fvs, gallery_fvs = self._expand(queries_fvs, gallery_fvs)
        distances, indices = ops_eval.pairdist_topk(queries_fvs.contiguous(), gallery_fvs.contiguous(), k, metric="cosine",
                                                    precision=self.precision, normalize=True)
        return indices, distances

    def calculateMetrics(self, distmat, queries, gallery):
        """validateModels.py:61-76 -> torchreid.metrics.evaluate_rank(distmat, q_pids, g_pids, q_camids, g_camids,
        use_metric_cuhk03=False)."""
        if not isinstance(distmat, torch.Tensor):
            distmat = torch.as_tensor(np.asarray(distmat))
        distmat = distmat.to(torch.device("cuda", getattr(self, "gpu_index", 0)), dtype=torch.float32).contiguous()
        ranks = [1, 5, 10]
        print('Computing CMC and mAP ...')
        cmc, mAP = ops_eval.rank_eval(distmat, queries[:, 1], gallery[:, 1], queries[:, 2], gallery[:, 2], max_rank=50)
        print('** Results **')
        print('mAP: {:.2%}'.format(mAP))
        if self.report_minp:
            self.mINP = ops_eval.rank_eval_inp(distmat, queries[:, 1], gallery[:, 1], queries[:, 2], gallery[:, 2])
            print('mINP: {:.2%}'.format(self.mINP))
        print('Ranks:')
        for r in ranks:
            if r <= len(cmc):
                print('Rank-{:<3}: {:.2%}'.format(r, cmc[r - 1]))
        return cmc, mAP


class validateBRIAR(validateModels):
    """validateModels.validateBRIAR (validateModels.py:79-105): closed-set identification without camera filtering."""

    def calculateMetrics(self, distmat, queries, gallery):
        """validateModels.py:84-105: Rank-1/5/10/20 = the share of queries whose identity is among the identities of their 1/5/10/20
        nearest gallery entries; -> (list of the four rank values, 0).  The 20 nearest come from ops_eval.topk_rows instead of a full
        ``torch.argsort(distmat, dim=1)[:, :20]``.  Exactly equal distances are ordered by ascending gallery index here; torch.argsort is
        not stable by default and leaves that order unspecified, so on such ties the reference's own result is not defined either."""
        if not isinstance(distmat, torch.Tensor):
            distmat = torch.as_tensor(np.asarray(distmat))
        distmat = distmat.to(torch.device("cuda", getattr(self, "gpu_index", 0)), dtype=torch.float32)
        nq = queries.shape[0]
        gt = queries[:, 1].reshape(nq, 1)
        cmc = []
        ranks = [1, 5, 10, 20]
        print('Computing CMC and mAP ...')
        _, ranked_idx = ops_eval.topk_rows(distmat, 20)
        predicted = gallery[:, 1][ranked_idx.cpu().numpy()]
        matching = gt == predicted
        print('** Results **')
        print('Ranks:')
        for r in ranks:
            rank_value = np.mean(np.sum(matching[:, :r], axis=1) > 0)
            print('Rank-{:<3}: {:.2%}'.format(r, rank_value))
            cmc.append(rank_value)
        return cmc, 0


class MSMT17_validator:
    """validateModels.MSMT17_validator (validateModels.py:120-190): MSMT17's train/val balanced-accuracy validation.  mainKIT.main only
    builds it when ``dataset == 'MSMT17'`` (mainKIT.py:122-124); that dataset branch is outside the scope table.  The
    name exists so that ``from validateModels import validationManager, MSMT17_validator`` (mainKIT.py:28) keeps importing."""

    def __init__(self, train_images, val_images, trainer, dir_to_save):
        raise NotImplementedError("MSMT17_validator is out of scope of this build (SURVEY.md 2.1)")


class validationManager:

    @staticmethod
    def getValidator(name):
        """validateModels.py:108-118; the MSMT17 validator is outside the scope table."""
        if name == "MSMT17":
            raise NotImplementedError("validator for %s is out of scope of this build (SURVEY.md 2.1)" % name)
        if name == "BRIAR":
            return validateBRIAR()
        return validateModels()
