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
    templates = None              # setTemplates
    template_rows = None          # (query rows, gallery rows) the metrics of the last templated validate / retrieve ran on
    report_open_set = False       # True: calculateMetrics also computes FNIR at fixed FPIR on identities, prints it and leaves it in self.open_set
    open_set_fpirs = (1e-1, 1e-2, 1e-3)
    open_set_ranks = (1, 20)

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

    def setTemplates(self, query=None, gallery=None, pooling="mean", linkage=None):
        """Template evaluation: a set of rows stands for one search unit (BRIAR templates, video tracklets, Market-1501 multi-query).
        ``query`` / ``gallery``: None (every row its own template), a column index or a tuple of column indices of the subset array
        (``(1, 2)`` = by pid and camera), or a callable from the subset to the keys (``ops_eval.template_index``).  ``linkage=None``: the
        features are pooled per template (``ops_eval.pool_templates``, ``pooling`` = "mean" / "max" / "magnitude" / "unit_mean") before
        query expansion and ``distance``.  ``linkage`` = "min" / "mean" / "max": ``distance`` becomes ``ops_eval.link_templates`` over the
        features permuted so that templates are contiguous (re-ranking uses the same linkage for its q-q and g-g blocks).  The metrics
        run on one row per template, that of its first member, kept in ``self.template_rows``; members whose camera ids disagree give a
        camera id that equals no camera.  ``setTemplates()`` switches it off.  Without this call nothing changes."""
        if pooling not in ("mean", "max", "magnitude", "unit_mean"):
            raise ValueError("setTemplates: pooling must be 'mean', 'max', 'magnitude' or 'unit_mean', got %r" % (pooling,))
        if linkage not in (None, "min", "mean", "max"):
            raise ValueError("setTemplates: linkage must be None, 'min', 'mean' or 'max', got %r" % (linkage,))
        for name, spec in (("query", query), ("gallery", gallery)):
            cols = spec if isinstance(spec, tuple) else (spec,)
            if spec is None or callable(spec):
                continue
            if not cols or not all(isinstance(c, (int, np.integer)) and not isinstance(c, bool) and c >= 0 for c in cols):
                raise ValueError("setTemplates: %s must be None, a column index, a tuple of column indices or a callable, got %r" % (name, spec))
        if query is None and gallery is None:
            self.templates = None
            self.template_rows = None
            return
        self.templates = dict(query=query, gallery=gallery, pooling=pooling, linkage=linkage)

    def _check_templates(self, who):
        """Refusals of the template switch, raised before any feature is extracted."""
        if self.templates is None:
            return
        if self.templates["linkage"] is not None:
            if self.query_expansion is not None:
                raise ValueError("%s: query expansion works on one feature row per search unit; with linkage=%r a template keeps all its "
                                 "rows (use pooling, or setQueryExpansion(None))" % (who, self.templates["linkage"]))
            if who == "retrieve":
                raise NotImplementedError("retrieve: top-k retrieval without the matrix is not built for linkage=%r; use validate(), or "
                                          "pooled templates" % (self.templates["linkage"],))

    @staticmethod
    def _template_side(subset, spec):
        """-> (order, bounds, rows, mixed): the grouping of ``subset`` by ``spec``, one row per template (its first member's) and the
        templates whose members' camera ids disagree.  None for a side without templates."""
        if spec is None:
            return None
        subset = np.asarray(subset)
        if callable(spec):
            keys = spec(subset)
        else:
            keys = tuple(subset[:, c] for c in (spec if isinstance(spec, tuple) else (spec,)))
        order, bounds, first = ops_eval.template_index(keys if isinstance(keys, tuple) else np.asarray(keys))
        if order.size != len(subset):
            raise ValueError("setTemplates: the keys describe %d rows, the subset has %d" % (order.size, len(subset)))
        rows = subset[first].copy()
        cams = subset[order, 2]
        t_of = np.repeat(np.arange(first.size), np.diff(bounds))
        mixed = np.zeros(first.size, dtype=bool)
        mixed[t_of[cams != rows[t_of, 2]]] = True
        return order, bounds, rows, mixed

    def _template_sides(self, queries, gallery):
        """Both sides' groupings; the camera id of a mixed-camera template becomes a value no row of either side carries (one for the
        query side, another for the gallery side), so that the camera filter of the ranking never removes such a template."""
        sides = [self._template_side(queries, self.templates["query"]), self._template_side(gallery, self.templates["gallery"])]
        rows = [np.asarray(queries) if sides[0] is None else sides[0][2], np.asarray(gallery) if sides[1] is None else sides[1][2]]
        all_cams = np.concatenate([np.asarray(queries)[:, 2], np.asarray(gallery)[:, 2]])
        for i, tag in enumerate(("q", "g")):
            if sides[i] is None or not sides[i][3].any():
                continue
            r = rows[i]
            if r.dtype.kind in "US":
                mark = "mixed-" + tag
                while mark in set(all_cams.tolist()):
                    mark += "*"
                if r.dtype.kind == "S":
                    mark = mark.encode()
                r = r.astype("%s%d" % (r.dtype.kind, max(r.dtype.itemsize // (4 if r.dtype.kind == "U" else 1), len(mark))))
            elif r.dtype.kind == "O":
                mark = ("mixed", tag)
            else:
                mark = all_cams.max().item() + 1 + i
                if r.dtype.kind in "iu":             # wide enough for the mark whatever the subset's integer type
                    r = r.astype(np.int64)
            r[sides[i][3], 2] = mark
            rows[i] = r
        return sides, rows

    def _template_features(self, sides, queries_fvs, gallery_fvs):
        """Pooled features (linkage None), or the features permuted so that templates are contiguous, with the bounds ``_distance`` needs."""
        fvs, bounds = [queries_fvs, gallery_fvs], [None, None]
        linkage = self.templates["linkage"]
        for i, side in enumerate(sides):
            if side is None:
                if linkage is not None:
                    bounds[i] = np.arange(fvs[i].shape[0] + 1, dtype=np.int32)
                continue
            order, b = side[0], side[1]
            if linkage is None:
                fvs[i] = ops_eval.pool_templates(fvs[i].contiguous(), order, b, self.templates["pooling"])
            else:
                fvs[i] = fvs[i].index_select(0, torch.from_numpy(order.astype(np.int64)).to(fvs[i].device))
                bounds[i] = b
        return fvs[0], fvs[1], bounds[0], bounds[1]

    def _distance(self, a_fvs, b_fvs, a_bounds=None, b_bounds=None):
        if a_bounds is None:
            return self.distance(a_fvs, b_fvs)
        return ops_eval.link_templates(a_fvs, b_fvs, a_bounds, b_bounds, linkage=self.templates["linkage"], metric="cosine",
                                       precision=self.precision, normalize=True)

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
        self._check_templates("validate")
        model.eval()
        queries_fvs = self._features(queries, model)
        gallery_fvs = self._features(gallery, model)
        q_bounds = g_bounds = None
        if self.templates is not None:           # from here on a row is a template: features, metrics and the returned matrix
            sides, (queries, gallery) = self._template_sides(queries, gallery)
            self.template_rows = (queries, gallery)
            queries_fvs, gallery_fvs, q_bounds, g_bounds = self._template_features(sides, queries_fvs, gallery_fvs)
        queries_fvs, gallery_fvs = self._expand(queries_fvs, gallery_fvs)
        distmat = self._distance(queries_fvs, gallery_fvs, q_bounds, g_bounds)
        if getattr(self, "rerank", False):
            # validateModels.py:49-53 (commented out in the reference): every block is the same cosine distance, so the three agree
            print('Applying person re-ranking ...')
            distmat_qq = self._distance(queries_fvs, queries_fvs, q_bounds, q_bounds)
            distmat_gg = self._distance(gallery_fvs, gallery_fvs, g_bounds, g_bounds)
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
        if self.templates is not None:         # likewise
            raise NotImplementedError("validate_sharded: a template's members may lie in different gallery shards; "
                                      "use validate(), or setTemplates()")
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
        ties by ascending gallery index.  The distances are bitwise the entries ``validate`` would return in its matrix.  Under
        ``setTemplates`` with pooling the queries are query templates and the indices number the gallery templates
        (``self.template_rows``)."""
        self._check_templates("retrieve")
        model.eval()
        queries_fvs = self._features(queries, model)
        gallery_fvs = self._features(gallery, model)
        if self.templates is not None:
            sides, self.template_rows = self._template_sides(queries, gallery)
            self.template_rows = tuple(self.template_rows)
            queries_fvs, gallery_fvs, _, _ = self._template_features(sides, queries_fvs, gallery_fvs)
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
        self._report_open_set(distmat, queries, gallery)
        return cmc, mAP

    def _report_open_set(self, distmat, queries, gallery):
        """report_open_set: FNIR at fixed FPIR over identities (ops_eval.open_set_metrics; no camera filter, every gallery row a
        candidate), printed after the closed-set lines and left in ``self.open_set``."""
        if not self.report_open_set:
            return
        self.open_set = ops_eval.open_set_metrics(distmat, queries[:, 1], gallery[:, 1], self.open_set_fpirs, self.open_set_ranks)
        for f in self.open_set_fpirs:
            for r in self.open_set_ranks:
                print('FNIR@FPIR={:g} Rank-{:<3}: {:.2%}'.format(f, r, self.open_set["fnir"][(f, r)]))


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
        self._report_open_set(distmat, queries, gallery)
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
