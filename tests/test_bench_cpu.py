"""bench.py's command line (no GPU): a plain run is the headline alone, --full adds every measurement of its own."""
import bench


def test_plain_run_is_the_default():
    a = bench.parse(["--steps", "20", "--warmup", "5"])
    assert a.full is False and a.steps == 20 and a.warmup == 5
    assert a.no_extras is False and a.no_cpu_baseline is False


def test_full_and_its_opt_outs():
    a = bench.parse(["--full", "--no-extras", "--no-cpu-baseline", "--sizes", "128", "--slab-sizes", "64"])
    assert a.full is True and a.no_extras is True and a.no_cpu_baseline is True
    assert a.sizes == "128" and a.slab_sizes == "64"
