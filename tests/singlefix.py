"""TEST INFRASTRUCTURE for the single-variable output tests (test_single_outputs.py, test_gpu_single_outputs.py): reads
tests/golden/single_*.npz (written by tests/golden/make_golden_single.py from the reference's own executables).  Every comparison
is byte for byte."""
import importlib
import json
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
DECKS = os.path.join(ROOT, "atmospheric-athena_amd", "decks")
NGHOST = 4

HYDRO = ["single_blast_16x12x8_s2", "single_blast_67x12x8_s2", "single_blast2d_24x20_s3"]
SPHERE = "single_ioniz_sphere_20x20x20_s3"


def pkg(name=""):
    return importlib.import_module("atmospheric-athena_amd" + ("." + name if name else ""))


class Fixture:
    def __init__(self, name):
        self.name = name
        z = self.z = np.load(os.path.join(GOLDEN, name + ".npz"))
        self.nx = tuple(int(v) for v in z["nx"])
        self.problem = str(z["problem"])
        self.nlim = int(z["nlim"])
        self.blocks = json.loads(str(z["blocks"]))
        self.paths = [str(p) for p in z["paths"]]
        self.overrides = [str(v) for v in z["overrides"]]

    def par(self):
        """our deck with the run's <outputN> blocks"""
        text = open(os.path.join(DECKS, "athinput." + self.problem)).read()
        text = re.sub(r"(?ms)^<output\d+>.*?(?=^<|\Z)", "", text)
        text = re.sub(r"(?m)^maxout\s*=.*$", "maxout = %d" % max(int(k) for k in self.blocks), text, count=1)
        for n, kv in sorted(self.blocks.items(), key=lambda t: int(t[0])):
            text += f"\n<output{n}>\n" + "".join(f"{k} = {v}\n" for k, v in kv.items())
        return pkg("athinput").ParTable.from_text(text).cmdline(self.overrides)

    def run_config(self, par=None):
        return pkg("config").from_par(par or self.par(), "blast" if self.problem == "blast2d" else self.problem)   # (the deck's name / the generator's)

    def outputs(self, rundir, par=None, **kw):
        return pkg("outputs").OutputSet.from_par(par or self.par(), 0.0, str(rundir), single=True, **kw)

    def nums(self):
        return sorted(int(p.split(".")[1]) for p in self.paths if p.endswith(".rst"))

    def file(self, rel):
        return self.z["file_%d" % self.paths.index(rel)].tobytes()

    def state(self, num):
        """(key -> array, time) of the restart dump number `num`"""
        i = next(i for i, p in enumerate(self.paths) if p.endswith(".rst") and int(p.split(".")[1]) == num)
        return {k: self.z[f"rst_{i}_{k}"] for k in ("U", "ef") if f"rst_{i}_{k}" in self.z}, float(self.z[f"rst_{i}_time"])

    def block_with_ghosts(self, num):
        """the state of output `num` as a host block with its ghost zones: every boundary of the blast decks is periodic (bc 4),
        and bvals_mhd has run in front of every output"""
        U = self.state(num)[0]["U"][..., :5]
        pad = [(NGHOST, NGHOST) if n > 1 else (0, 0) for n in U.shape[:3]] + [(0, 0)]
        return np.pad(U, pad, mode="wrap")

    def singles(self):
        return [p for p in self.paths if not p.endswith(".rst")]


def tree(rundir):
    return sorted(os.path.relpath(os.path.join(dp, f), str(rundir)) for dp, _, fs in os.walk(str(rundir)) for f in fs)


def compare_singles(fx, rundir, nums=None):
    """every single-variable file of the fixture (of the outputs `nums`): the same names, the same count, the same bytes"""
    want = [p for p in fx.singles() if nums is None or int(p.split(".")[1]) in nums]
    got = [p for p in tree(rundir) if not p.endswith(".rst")]
    assert got == want, (got, want)
    for rel in want:
        ours = open(os.path.join(str(rundir), rel), "rb").read()
        ref = fx.file(rel)
        if ours != ref:
            a, b = np.frombuffer(ours, np.uint8), np.frombuffer(ref, np.uint8)
            n = min(a.size, b.size)
            bad = np.nonzero(a[:n] != b[:n])[0]
            raise AssertionError(f"{fx.name}:{rel}: {len(ours)} bytes against {len(ref)}, {bad.size} differ"
                                 + (f", first at {int(bad[0])}" if bad.size else ""))


class HostEngine:
    """an engine without a device for Driver.write_single: a host block with ghost zones (and EdgeFlux)"""
    def __init__(self, U=None, ef=None):
        self.U, self.ef = U, ef

    def download(self): return self.U
    def download_edgeflux(self): return self.ef
    def close(self): pass


def host_driver(fx, par=None):
    run = fx.run_config(par)
    return pkg("driver").Driver(run, engine_factory=lambda grid: HostEngine())
