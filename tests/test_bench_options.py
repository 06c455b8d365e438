"""bench.py's two kinds of run: a plain one times the headline alone; --full adds every secondary measurement."""
import bench

ALL_LEGS = {"mixed", "train", "post", "sweep", "cpu_baseline"}


def test_plain_run_times_the_headline_alone():
    args = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert not args.full and args.modes == ["fp32"]
    assert bench.secondary_legs(args, rank=0, world=1) == set()


def test_full_run_measures_everything_else():
    args = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
    assert args.modes == ["fp32", "bf16x6", "bf16x3"]
    assert bench.secondary_legs(args, rank=0, world=1) == ALL_LEGS
    # several GPUs: the other modes are timed on every rank, the one-GPU legs stay out
    assert bench.secondary_legs(args, rank=0, world=8) == set()


def test_no_options_leave_legs_out_of_a_full_run():
    args = bench.parse_args(["--full", "--no-sweep", "--no-cpu-baseline", "--modes", "bf16x3"])
    assert args.modes == ["bf16x3"]
    assert bench.secondary_legs(args, rank=0, world=1) == {"train", "post"}  # no fp32: no bf16x3-attention leg
    args = bench.parse_args(["--modes", "fp32,bf16x3", "--no-train"])  # explicit modes hold in a plain run too
    assert args.modes == ["fp32", "bf16x3"] and bench.secondary_legs(args, rank=0, world=1) == set()
