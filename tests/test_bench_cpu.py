"""CPU-only tests of bench.py's command line: a plain run measures the headline alone, --full adds every extra measurement
that its --no-* flag leaves on."""
import bench


def test_plain_run_measures_only_the_headline():
    for argv in (["--gpus", "1", "--steps", "3", "--warmup", "1"], ["--dump-outputs", "out"], ["--force-dp"]):
        assert bench.extras(bench.parse_args(argv)) == frozenset(), argv


def test_full_measures_every_extra_its_flag_leaves_on():
    assert bench.extras(bench.parse_args(["--full"])) == frozenset(bench.EXTRAS)
    for k in bench.EXTRAS:                       # every extra has a --no-* flag that leaves it out of a --full run
        flag = "--no-" + k.replace("_", "-")
        assert bench.extras(bench.parse_args(["--full", flag])) == frozenset(bench.EXTRAS) - {k}, flag
