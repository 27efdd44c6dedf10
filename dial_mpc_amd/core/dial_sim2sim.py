"""``dial-mpc-sim2sim``: the plant (dial-mpc-sim) and the planner (dial-mpc-plan) as two child processes, the way the reference's
dial_mpc/core/dial_sim2sim.py starts them -- but with ``sys.executable -m`` (no installed console script needed), started once
the plant's shared-memory segments exist instead of after a fixed 2 s, and supervised: when either child exits, the other is
interrupted (SIGINT, then killed if it does not stop), and the first non-zero exit status is returned.

Arguments are forwarded to both children (--config / --example / --list-examples, --custom-env, --shm-prefix); --duration goes to
the plant only.
"""
from __future__ import annotations

import argparse
import os
import signal
import subprocess
import sys
import time

SEGMENTS = ("time_shm", "state_shm", "acts_shm", "refs_shm", "plan_time_shm", "tau_shm")


def _segments_exist(prefix: str) -> bool:
    return all(os.path.exists(os.path.join("/dev/shm", prefix + name)) for name in SEGMENTS)


def _stop(proc: subprocess.Popen, grace: float = 20.0):
    if proc.poll() is not None:
        return
    proc.send_signal(signal.SIGINT)   # (both processes clean up on KeyboardInterrupt: the plant saves its record and unlinks)
    try:
        proc.wait(grace)
    except subprocess.TimeoutExpired:
        proc.kill()
        proc.wait()


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    parser = argparse.ArgumentParser()
    group = parser.add_mutually_exclusive_group(required=True)
    group.add_argument("--config", type=str, default=None)
    group.add_argument("--example", type=str, default=None)
    group.add_argument("--list-examples", action="store_true")
    parser.add_argument("--custom-env", type=str, default=None)
    parser.add_argument("--shm-prefix", type=str, default="")
    parser.add_argument("--duration", type=float, default=None, help="Seconds of simulated time (plant only; default: forever)")
    parser.add_argument("--startup-timeout", type=float, default=300.0, help="Seconds to wait for the plant's segments")
    args = parser.parse_args(argv)
    common = []
    if args.config is not None:
        common += ["--config", args.config]
    elif args.example is not None:
        common += ["--example", args.example]
    else:
        common += ["--list-examples"]
    if args.custom_env is not None:
        common += ["--custom-env", args.custom_env]
    common += ["--shm-prefix", args.shm_prefix]
    if args.list_examples:
        return subprocess.call([sys.executable, "-m", "dial_mpc_amd.deploy.dial_sim"] + common)
    sim_args = common + (["--duration", str(args.duration)] if args.duration is not None else [])
    sim = subprocess.Popen([sys.executable, "-m", "dial_mpc_amd.deploy.dial_sim"] + sim_args)
    plan = None
    try:
        deadline = time.time() + args.startup_timeout
        while not _segments_exist(args.shm_prefix):
            if sim.poll() is not None:
                return sim.returncode or 1
            if time.time() > deadline:
                print("[dial-mpc-sim2sim] the plant did not create its shared-memory segments in time", file=sys.stderr)
                return 1
            time.sleep(0.05)
        plan = subprocess.Popen([sys.executable, "-m", "dial_mpc_amd.deploy.dial_plan"] + common)
        while sim.poll() is None and plan.poll() is None:
            time.sleep(0.05)
        first = sim if sim.poll() is not None else plan
        other = plan if first is sim else sim
        _stop(other)
        codes = [first.returncode, other.returncode]
        return next((c for c in codes if c != 0), 0)
    except KeyboardInterrupt:
        return 0
    finally:
        for p in (plan, sim):
            if p is not None:
                _stop(p)


if __name__ == "__main__":
    sys.exit(main())
