"""bench.py, unchanged, with Config::device_pnp forced ON for every key-frame pipeline it makes: the switch is off by default, so the A/B of DESIGN.md section 0.2d
runs `python bench.py ...` for the off case and `python tools/bench_device_pnp.py ...` (the same arguments) for the on case.  The switch is set through the C
entry (omni_pipeline_set_device_pnp, lib/libomni_host_pnp.so) right after each pipeline is created; the device / host candidate counters of the pipelines are
printed to stderr when they are closed, so that a run shows that the device did serve the with_geometry leg's candidates."""
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import omni_loader  # noqa: E402

omni_loader.load()
from omni_swarm_amd import pipeline  # noqa: E402

_init, _close = pipeline.KeyframePipeline.__init__, pipeline.KeyframePipeline.close


def init_with_device_pnp(self, *args, **kwargs):
    _init(self, *args, **kwargs)
    self.set_device_pnp(True)


def close_and_report(self):
    if getattr(self, "h", None):
        on, dev, host = self.device_pnp()
        print(f"[bench_device_pnp] pipeline closed: device_pnp {on}, candidates on the device {dev}, handed back to the host {host}", file=sys.stderr)
    _close(self)


pipeline.KeyframePipeline.__init__ = init_with_device_pnp
pipeline.KeyframePipeline.close = close_and_report
sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[1:]
runpy.run_path(sys.argv[0], run_name="__main__")
