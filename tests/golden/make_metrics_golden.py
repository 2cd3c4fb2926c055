"""Writes tests/golden/metrics.npz: inputs and outputs of the reference's
smcdet/metrics.py (match_catalogs, compute_precision_recall_f1), run on the
CPU from a checkout of the reference (timwhite0/smcdet):

    python tests/golden/make_metrics_golden.py /path/to/reference [seed]

The file holds data only.  Cases (tests/_metrics_oracle.synth_case builds the
catalogs and keeps the decision margins; see its docstring):

  small  T=24 tiles on an 8x8 frame, St=Se=10, N=64 catalogs per tile, M=32,
         locs_tol = mags_tol = 0.5, mag_bins = arange(16, 24.5, 0.5).  The
         reference runs under torch.manual_seed(seed); its catalog choice is
         recovered by replaying the same torch.randint calls under that seed.
  bin2   the same data with the drivers' mag_bins = arange(14.0, 22.5, 8)
         and index = arange over the first 8 catalogs.  The reference always
         draws its catalogs, so it is called once per catalog on a
         single-catalog slice, where its randint(0, 1) can only pick that one.
  prf    compute_precision_recall_f1 on the small outputs, and on a copy in
         which one bin's totals are zero (nan_to_num), plus the converters.

ref_is_lex [T,M]: where the reference's bucketed outputs equal the oracle's
(the exact lexicographic optimum, tests/_metrics_oracle.py).  The generator
refuses a seed for which more than 2 % of the small problems differ.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import _metrics_oracle as O  # noqa: E402

LOCS_TOL = MAGS_TOL = 0.5
BINS_SMALL = torch.arange(16, 24.5, 0.5)
BINS_2 = torch.arange(14.0, 22.5, 8)
T, N, S, M, FRAME = 24, 64, 10, 32, 8.0
M2 = 8


def ref_is_lex(ref, ora):
    return np.logical_and.reduce([(r == o).all(-1) for r, o in zip(ref, ora)])


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, sys.argv[1])
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    from smcdet.metrics import compute_precision_recall_f1, match_catalogs
    from utils.sdss import convert_mag_to_nmgy, convert_nmgy_to_mag

    torch.set_default_dtype(torch.float32)
    case = O.synth_case(seed, T, N, S, S, FRAME, LOCS_TOL, MAGS_TOL,
                        [BINS_SMALL.numpy(), BINS_2.numpy()])
    tens = {k: torch.from_numpy(v) for k, v in case.items()}
    args = (tens["true_counts"], tens["true_locs"], tens["true_fluxes"], tens["est_counts"],
            tens["est_locs"], tens["est_fluxes"])

    # small: the reference's own draws, replayed
    torch.manual_seed(seed)
    ref = [x.numpy() for x in match_catalogs(*args, M, LOCS_TOL, MAGS_TOL, BINS_SMALL)]
    torch.manual_seed(seed)
    index = torch.stack([torch.randint(0, N, [M]) for _ in range(T)]).numpy()
    ora = O.match_catalogs(*case.values(), index, LOCS_TOL, MAGS_TOL, BINS_SMALL.numpy())
    lex = ref_is_lex(ref, ora[:4])
    miss = 1.0 - lex.mean()
    print(f"small: reference != lexicographic optimum in {int((~lex).sum())} of {lex.size} "
          f"problems ({100 * miss:.2f} %)")
    assert miss <= 0.02, "choose another seed"
    for r, o in zip((ref[0], ref[2]), (ora[0], ora[2])):
        assert np.array_equal(r, o)
    for r, o in zip((ref[1], ref[3]), (ora[1], ora[3])):
        assert np.array_equal(r.sum(-1), o.sum(-1))

    # bin2: catalogs 0..7 in order; one reference call per (tile, catalog) so
    # that its randint(0, 1) can only pick that catalog
    index2 = np.tile(np.arange(M2), (T, 1))
    ref2 = [np.zeros((T, M2, len(BINS_2)), np.float32) for _ in range(4)]
    for j in range(M2):
        out = match_catalogs(args[0], args[1], args[2], args[3][:, j:j + 1], args[4][:, j:j + 1],
                             args[5][:, j:j + 1], 1, LOCS_TOL, MAGS_TOL, BINS_2)
        for k in range(4):
            ref2[k][:, j] = out[k][:, 0].numpy()
    ora2 = O.match_catalogs(*case.values(), index2, LOCS_TOL, MAGS_TOL, BINS_2.numpy())
    lex2 = ref_is_lex(ref2, ora2[:4])
    print(f"bin2: reference != lexicographic optimum in {int((~lex2).sum())} of {lex2.size}")

    # prf: the reference's precision / recall / F1, and a copy with an empty bin
    prf = [x.numpy() for x in compute_precision_recall_f1(*[torch.from_numpy(r) for r in ref])]
    zero = [r.copy() for r in ref]
    zb = int(np.argmax(ref[0].sum((0, 1))))  # a populated bin, emptied
    for z in zero:
        z[..., zb] = 0
    prf0 = [x.numpy() for x in compute_precision_recall_f1(*[torch.from_numpy(z) for z in zero])]
    mags = torch.linspace(14, 24, 41)
    nmgy = convert_mag_to_nmgy(mags)

    out = dict(seed=seed, locs_tol=LOCS_TOL, mags_tol=MAGS_TOL, mag_bins=BINS_SMALL.numpy(),
               mag_bins2=BINS_2.numpy(), index=index, index2=index2, ref_is_lex=lex,
               ref_is_lex2=lex2, prf_zero_bin=zb, conv_mags=mags.numpy(), conv_nmgy=nmgy.numpy(),
               conv_mags_back=convert_nmgy_to_mag(nmgy).numpy(), **case)
    names = ("true_total", "true_matches", "est_total", "est_matches")
    for k, name in enumerate(names):
        out[f"ref_{name}"] = ref[k]
        out[f"ref2_{name}"] = ref2[k]
        out[f"prf0_in_{name}"] = zero[k]
    for k, name in enumerate(("precision", "recall", "f1")):
        out[f"prf_{name}"] = prf[k]
        out[f"prf0_{name}"] = prf0[k]
    path = os.path.join(HERE, "metrics.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
