"""smcdet_amd.images.generate_images (reference images.py:178-228) on the CPU:
its prune and compaction against a few lines of numpy, with stub Prior /
ImageModel objects that return fixed tensors."""
import numpy as np
import pytest
import torch

from smcdet_amd.images import generate_images

FLUX_T, LO, HI = 5.0, 0.0, 8.0


class StubPrior:
    def __init__(self, counts, locs, fluxes):
        self.cat = [torch.as_tensor(np.asarray(x, np.float32))[None, None]
                    for x in (counts, locs, fluxes)]
        self.asked = None

    def sample(self, num_catalogs=1):
        self.asked = num_catalogs
        return self.cat


class StubModel:
    H, W = 3, 4

    def sample(self, locs, fluxes):
        n = locs.shape[2]
        self.seen = (locs, fluxes)
        # image n is filled with n + 1: the output order of the images shows
        return (torch.arange(1, n + 1, dtype=torch.float32)
                * torch.ones(1, 1, self.H, self.W, n))


def numpy_prune(locs, fluxes):
    """Kept sources (strictly inside (LO, HI)^2, flux strictly above FLUX_T)
    moved to the front in their order, zeros behind."""
    n, s, _ = locs.shape
    pc = np.zeros(n, np.int64)
    pl, pf = np.zeros_like(locs), np.zeros_like(fluxes)
    for i in range(n):
        keep = [j for j in range(s)
                if LO < locs[i, j, 0] < HI and LO < locs[i, j, 1] < HI and fluxes[i, j] > FLUX_T]
        pc[i] = len(keep)
        pl[i, :len(keep)] = locs[i, keep]
        pf[i, :len(keep)] = fluxes[i, keep]
    return pc, pl, pf


CATALOGS = {
    # each row: (h, w, flux)
    "edges": [[(0.0, 4.0, 9.0), (3.0, 8.0, 9.0), (3.0, 4.0, 5.0), (1e-3, 7.999, 5.001)],
              [(8.0, 8.0, 9.0), (2.0, 2.0, 6.0), (-0.5, 4.0, 9.0), (7.0, 1.0, 7.0)],
              [(4.0, 4.0, 4.999), (4.0, 0.0, 9.0), (6.5, 6.5, 50.0), (8.5, 1.0, 9.0)]],
    "all_pruned": [[(-1.0, 4.0, 9.0), (3.0, 9.0, 9.0), (3.0, 4.0, 1.0)],
                   [(0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)]],
    "none_pruned": [[(1.0, 2.0, 6.0), (3.0, 4.0, 7.0), (5.0, 6.0, 8.0)],
                    [(7.5, 0.5, 5.5), (0.5, 7.5, 9.5), (4.0, 4.0, 100.0)]],
    "one_catalog": [[(9.0, 9.0, 9.0), (1.0, 1.0, 9.0)]],
}


@pytest.mark.parametrize("name", list(CATALOGS))
def test_generate_images_prunes_and_compacts(name):
    cat = np.array(CATALOGS[name], np.float32)               # [n, S, 3]
    locs, fluxes = cat[..., :2], cat[..., 2]
    counts = (fluxes > 0).sum(-1).astype(np.float32)
    prior, model = StubPrior(counts, locs, fluxes), StubModel()
    n = cat.shape[0]
    out = generate_images(prior, model, FLUX_T, LO, HI, num_images=n)
    uc, ul, uf, pc, pl, pf, images = [np.asarray(o) for o in out]
    assert prior.asked == n
    # the model rendered the unpruned catalogs
    assert model.seen[0] is prior.cat[1] and model.seen[1] is prior.cat[2]
    np.testing.assert_array_equal(uc, counts)
    np.testing.assert_array_equal(ul, locs)
    np.testing.assert_array_equal(uf, fluxes)
    rc, rl, rf = numpy_prune(locs, fluxes)
    np.testing.assert_array_equal(pc, rc)
    np.testing.assert_array_equal(pl, rl)
    np.testing.assert_array_equal(pf, rf)
    assert images.shape == (n, StubModel.H, StubModel.W)
    np.testing.assert_array_equal(images[:, 0, 0], np.arange(1, n + 1))
    if name == "all_pruned":
        assert not pc.any() and not pl.any() and not pf.any()
    if name == "none_pruned":
        np.testing.assert_array_equal(pl, locs)
        assert (pc == cat.shape[1]).all()
    if name == "edges":
        # on a threshold is out: only the strictly inside, strictly brighter stay
        np.testing.assert_array_equal(pc, [1, 2, 1])
