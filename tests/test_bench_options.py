"""bench.py's command line on CPU: a plain run times the headline workload alone; `--full` adds the CPU baseline and, on the
default workload at one GPU, the `other_configs` sub-lines, as a default invocation did before the option existed."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _extras(argv, world=1):
    import bench
    return bench.extras(bench.parse(argv), world)


def test_plain_run_has_no_extras():
    assert _extras(["--gpus", "1", "--steps", "20", "--warmup", "5"]) == (False, False)
    assert _extras(["--dump-outputs", "out"]) == (False, False)
    assert _extras(["--dtype", "bf16", "--emb", "300"]) == (False, False)
    assert _extras(["--review_net_only", "--batch", "32"]) == (False, False)


def test_full_runs_what_a_default_invocation_ran():
    assert _extras(["--full", "--gpus", "1", "--steps", "20", "--warmup", "5"]) == (True, True)
    assert _extras(["--full", "--dump-outputs", "out"]) == (True, True)
    assert _extras(["--full", "--no-other-configs"]) == (False, True)
    assert _extras(["--full", "--no-cpu-baseline"]) == (True, False)
    # an explicit workload keeps its CPU baseline but has no sub-lines
    for flags in (["--dtype", "bf16", "--emb", "300"], ["--review_net_only", "--batch", "32"], ["--h2d"], ["--realistic"],
                  ["--views", "4"]):
        assert _extras(["--full"] + flags) == (False, True), flags
    # forward-only workloads have no training step to compare on the CPU
    assert _extras(["--full", "--eval"]) == (False, False)
    assert _extras(["--full", "--fwd-train"]) == (False, False)


def test_full_extras_are_single_gpu_only():
    assert _extras(["--full", "--gpus", "2"], world=2) == (False, False)
