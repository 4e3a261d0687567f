"""GPU: the BRIAR validator (validateModels.validateBRIAR.calculateMetrics, validateModels.py:79-105) against a restatement of the
reference's lines with torch.argsort, and validateModels.retrieve against tests/topk_ref.py on validate's own distance matrix."""
import numpy as np
import pytest
import torch

import topk_ref as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _briar_restated(distmat, queries, gallery):
    """validateModels.py:84-105 without the prints"""
    nq = queries.shape[0]
    gt = queries[:, 1].reshape(nq, 1)
    cmc = []
    ranks = [1, 5, 10, 20]
    ranked_idx = torch.argsort(distmat, dim=1)[:, :20]
    predicted = gallery[:, 1][ranked_idx]
    matching = gt == predicted
    for r in ranks:
        cmc.append(np.mean(np.sum(matching[:, :r], axis=1) > 0))
    return cmc, 0


def _rows(rng, n, n_ids):
    """[path, pid, camid] string rows as the reference's loaders build them"""
    return np.array([["img_%04d.jpg" % i, "%04d" % rng.integers(0, n_ids), "c%d" % rng.integers(0, 3)] for i in range(n)])


@pytest.mark.parametrize("nq,ng", [(37, 301), (9, 15)])
def test_briar_metrics_match_the_reference_lines(dev, nq, ng, capsys):
    from daliid_amd import validateModels as V
    rng = np.random.default_rng(nq + ng)
    distmat = torch.from_numpy(rng.uniform(0, 2, (nq, ng)).astype(np.float32))          # continuous: no ties
    queries, gallery = _rows(rng, nq, 12), _rows(rng, ng, 12)
    validator = V.validationManager.getValidator("BRIAR")
    assert isinstance(validator, V.validateBRIAR) and isinstance(validator, V.validateModels)
    validator.setParameters(64, 32, False, 0)
    cmc, mAP = validator.calculateMetrics(distmat.to(dev), queries, gallery)
    out = capsys.readouterr().out
    want, _ = _briar_restated(distmat, queries, gallery)
    assert mAP == 0 and len(cmc) == 4 and [float(c) for c in cmc] == [float(w) for w in want]
    assert 0 < want[3] and want[0] <= want[3]                                              # (the case is not degenerate)
    assert "Computing CMC and mAP ..." in out and "Rank-20 : {:.2%}".format(want[3]) in out
    cmc_host, _ = validator.calculateMetrics(distmat, queries, gallery)                 # a CPU tensor is copied to the device
    assert [float(c) for c in cmc_host] == [float(w) for w in want]


def test_retrieve_equals_topk_of_validates_matrix(dev):
    from daliid_amd import Encoders, synthetic, validateModels as V
    data = synthetic.SyntheticImages(n_ids=8, per_id=6, n_cams=3, seed=5, noise=0.4).install()
    try:
        online = Encoders._DataParallelShim(Encoders.ResNet50ReID(layers=(1, 1, 1, 1), width=32, seed=9)).eval()
        _, gallery, query = data.split(1)
        validator = V.validationManager.getValidator("Market")
        validator.setParameters(64, 32, False, 0)
        _, _, distmat = validator.validate(query, gallery, online)
        for k in (5, 50):
            indices, distances = validator.retrieve(query, gallery, online, k=k)
            wv, wi = T.topk(distmat.cpu().numpy(), min(k, len(gallery)))
            assert indices.dtype == torch.int32 and np.array_equal(indices.cpu().numpy(), wi)
            assert np.array_equal(distances.cpu().numpy().view(np.uint32), wv.view(np.uint32))
    finally:
        synthetic.SyntheticImages.uninstall()
