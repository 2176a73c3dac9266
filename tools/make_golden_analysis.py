"""Golden vectors of the reference's fastbox/analysis.py (interpolate_onto_grid, grid_catalogue) for
tests/test_regrid_cases_cpu.py and tests/test_regrid_gpu.py.  CPU only.  Loads the reference module by path (it needs only numpy
and SciPy), so it runs only where the reference sources are present; the output, data only, is committed under tests/golden/.

    python tools/make_golden_analysis.py <path of the reference's fastbox/analysis.py>

analysis_n16.npz holds: the 5 x 7 x 6 cube with one NaN voxel of tests/regrid_cases.py ('nan voxel') with its coordinates,
the reference's result on the 9 x 4 x 11 points of that case (rg_out, shape (4, 9, 11): the 'xy' order) and on the 16^3 points
of 'onto the box' (rg_box); 400 seeded positions over a little more than [0, 32)^3 with signed integer weights, and the
reference's grid_catalogue of them onto 16^3 with limits (0, 32) unweighted (gc_count) and weighted (gc_weighted), and onto
(3, 5, 7) with no limits given (gc_range, with its three grids gc_x, gc_y, gc_z)."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import regrid_cases as rc                                           # noqa: E402


def load_analysis(path):
    spec = importlib.util.spec_from_file_location("reference_analysis", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make(mod):
    cases = rc.regrid_cases()
    c, b = cases["nan voxel"], cases["onto the box"]
    out = dict(rg_field=c["field"], rg_x=c["coords_orig"][0], rg_y=c["coords_orig"][1], rg_z=c["coords_orig"][2],
               rg_xnew=c["coords_new"][0], rg_ynew=c["coords_new"][1], rg_znew=c["coords_new"][2],
               rg_out=mod.interpolate_onto_grid(c["field"], c["coords_orig"], c["coords_new"]),
               rg_box_xnew=b["coords_new"][0], rg_box_ynew=b["coords_new"][1], rg_box_znew=b["coords_new"][2],
               rg_box=mod.interpolate_onto_grid(c["field"], c["coords_orig"], b["coords_new"]))
    pos = rc.cloud(400, (32., 32., 32.))
    w = np.random.RandomState(9).randint(-7, 8, pos.shape[0]).astype(np.float64)
    lim = dict(xlim=(0., 32.), ylim=(0., 32.), zlim=(0., 32.), nx=16, ny=16, nz=16)
    out.update(gc_pos=pos, gc_w=w)
    out["gc_count"], _ = mod.grid_catalogue(pos[:, 0], pos[:, 1], pos[:, 2], **lim)
    out["gc_weighted"], _ = mod.grid_catalogue(pos[:, 0], pos[:, 1], pos[:, 2], w=w, **lim)
    out["gc_range"], (out["gc_x"], out["gc_y"], out["gc_z"]) = mod.grid_catalogue(pos[:, 0], pos[:, 1], pos[:, 2], nx=3, ny=5, nz=7)
    print("regrid: %d of %d NaN on the 9 x 4 x 11 points, %d of %d on the box; catalogue: %d of %d particles inside (0, 32)^3"
          % (np.isnan(out["rg_out"]).sum(), out["rg_out"].size, np.isnan(out["rg_box"]).sum(), out["rg_box"].size,
             out["gc_count"].sum(), pos.shape[0]))
    return out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    out = os.path.join(ROOT, "tests", "golden", "analysis_n16.npz")
    np.savez_compressed(out, **make(load_analysis(sys.argv[1])))
    print("wrote", out)


if __name__ == "__main__":
    main()
