"""bench.py's command line: a plain run is the headline only, --full is an explicit option (no GPU needed)."""
import bench


def test_full_is_off_by_default():
    a = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "2"])
    assert a.full is False and (a.gpus, a.steps, a.warmup) == (1, 3, 2)
    assert (a.size, a.model, a.dtype, a.mode, a.batch, a.eager) == (128, "UNet", "f32", "train", 1, False)


def test_full_and_the_flags_that_trim_it():
    a = bench.parse_args(["--full"])
    assert a.full and not a.no_cpu_baseline and not a.no_kernel_timer and not a.cpu_check_only
    a = bench.parse_args(["--full", "--no-cpu-baseline", "--no-kernel-timer"])
    assert a.full and a.no_cpu_baseline and a.no_kernel_timer
    # the trimming flags alone do not switch the extra legs on
    assert bench.parse_args(["--no-cpu-baseline"]).full is False
