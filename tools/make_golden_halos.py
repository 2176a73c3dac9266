"""Golden vectors of the reference's fastbox/halos.py (HaloDistribution.halo_count_field, realise_halo_catalogue) for
tests/test_halos_*.py.  Loads the reference module by path with pyccl stubbed as an empty module, so it runs only where the
reference sources are present; the outputs are committed under tests/golden/.

    python tools/make_golden_halos.py <path of the reference's fastbox/halos.py>

Each file halos_n<N>.npz holds, under the recorded seeds: L (3,), delta (N,N,N; fp32 values, the reference ran on them in
fp64), nbar_z (N,), bias,
counts (lognormal=False, np.random.seed(seed_counts)), counts_ln (lognormal=True, seed_counts_ln), cat (no scatter),
cat_scatter (scatter=True, np.random.seed(seed_cat))."""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_halos(path):
    import matplotlib
    matplotlib.use("Agg")
    sys.modules.setdefault("pyccl", types.ModuleType("pyccl"))
    spec = importlib.util.spec_from_file_location("reference_halos", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make(mod, N, L, seed, per_voxel):
    rs = np.random.RandomState(seed)
    delta = (0.6 * rs.standard_normal((N, N, N))).astype(np.float32).astype(np.float64)
    voxel_vol = L[0] * L[1] * L[2] / N ** 3.
    nbar_z = per_voxel * (1.2 + 0.8 * np.sin(np.arange(N) * 0.7)) / voxel_vol     # per_voxel halos per voxel, varying along z
    bias = 1.5
    box = types.SimpleNamespace(Lx=L[0], Ly=L[1], Lz=L[2], N=N)
    hd = mod.HaloDistribution(box, mass_range=(1e12, 1e15), mass_bins=10)
    seeds = dict(seed_counts=seed + 1, seed_counts_ln=seed + 2, seed_cat=seed + 3)
    np.random.seed(seeds["seed_counts"])
    counts = hd.halo_count_field(delta, nbar_z, bias)
    np.random.seed(seeds["seed_counts_ln"])
    counts_ln = hd.halo_count_field(delta, nbar_z, bias, lognormal=True)
    cat = hd.realise_halo_catalogue(counts)
    np.random.seed(seeds["seed_cat"])
    cat_scatter = hd.realise_halo_catalogue(counts, scatter=True)
    return dict(L=np.array(L, dtype=np.float64), delta=delta.astype(np.float32), nbar_z=nbar_z, bias=np.float64(bias),
                counts=counts.astype(np.int16),
                counts_ln=counts_ln.astype(np.int16), cat=cat, cat_scatter=cat_scatter, **{k: np.int64(v) for k, v in seeds.items()})


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    mod = load_halos(sys.argv[1])
    # the 32^3 file is kept sparse (0.2 halos per voxel) so that its catalogues stay small
    for N, L, seed, per_voxel in ((16, (300., 320., 340.), 101, 1.0), (32, (500., 500., 500.), 202, 0.2)):
        out = os.path.join(ROOT, "tests", "golden", "halos_n%d.npz" % N)
        np.savez_compressed(out, **make(mod, N, L, seed, per_voxel))
        print("wrote", out)


if __name__ == "__main__":
    main()
