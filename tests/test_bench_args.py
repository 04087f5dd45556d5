"""bench.py's options: a plain run times the steps and nothing else; --full adds the roofline, the CPU baseline and the 512^3 block."""
import bench

EXTRAS = ("no_cpu_baseline", "no_target_512", "no_solo_step", "no_live_pmc")


def test_plain_run_skips_every_extra():
    a = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert not a.full
    assert all(getattr(a, k) for k in EXTRAS)
    assert (a.gpus, a.steps, a.warmup) == (1, 3, 1)


def test_full_run_takes_every_extra_unless_skipped():
    a = bench.parse_args(["--full"])
    assert a.full and not any(getattr(a, k) for k in EXTRAS)
    a = bench.parse_args(["--full", "--no-target-512", "--no-live-pmc"])
    assert a.no_target_512 and a.no_live_pmc and not a.no_cpu_baseline and not a.no_solo_step


def test_counter_pass_child_is_a_plain_run(monkeypatch):
    """live_pmc's children run one step under rocprofv3 and print their line: plain runs, with no extras of their own under the profiler"""
    import shutil
    import subprocess
    cmds = []

    def fake_run(cmd, **kw):
        cmds.append(cmd)
        raise subprocess.TimeoutExpired(cmd, 0)

    for k in ("MER_BENCH_PMC_CHILD", "ROCPROFILER_REGISTER_FORCE_LOAD", "ROCP_TOOL_LIBRARIES", "ROCPROF_OUTPUT_PATH"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(shutil, "which", lambda name: "rocprofv3")
    monkeypatch.setattr(subprocess, "run", fake_run)
    traffic, why = bench.live_pmc("cfg3", 256, 512, 256, "brick27", "")
    assert traffic is None and "timed out" in why
    child = cmds[0][cmds[0].index("--") + 3:]              # after "--": python, bench.py, its arguments
    a = bench.parse_args(child)
    assert not a.full and (a.steps, a.warmup, a.options) == (1, 0, "pipes=1")
