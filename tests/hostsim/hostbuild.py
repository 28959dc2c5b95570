"""The one place that compiles the TEST-ONLY host builds under tests/hostsim/ (see hip_sim.hpp for what they are).

    from hostsim import hostbuild
    lib = hostbuild.load("em")              # a ctypes.CDLL, built if stale, one per process
    hostbuild.build_all()                   # every stale library, in parallel (what __graft_entry__.build() calls)

LIBS and DRIVERS are the tables: one row per library or program, its source and its flags.  A row lists no headers: g++
reports them (-MMD), and a product is fresh exactly when it, its dependency file (.d) and its stamp (.stamp) exist and the
stamp equals the digest of the command line and of the bytes of every dependency inside the repository.  Paths are kept
relative to the repository's root, so a tree copied elsewhere stays fresh; file times play no part.  A compile writes
temporary names and renames them into place, the stamp last, so a failed or interrupted one leaves the previous product.

    python tests/hostsim/hostbuild.py drivers

builds the four stand-alone driver programs with the host sanitizers (address, undefined), runs each and fails on a
non-zero exit.  They are ordinary host programs with a main of their own: nothing is loaded into Python and nothing is
preloaded.  The command is not a pytest test, carries no gpu mark and is for the machine without a GPU only.
"""
import ctypes
import hashlib
import os
import shlex
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
BUILD = os.path.join(HERE, "_build")

SHARED = ["-O2", "-std=c++17", "-fPIC", "-shared"]
EXACT = ["-ffp-contract=off"]                       # NumPy's roundings: no fused multiply-add
EXACT_EM = EXACT + ["-Wno-unknown-pragmas"]         # ... over the EM headers, which carry clang's unroll pragmas
# -fno-builtin: g++ merges sin(a) and cos(a) into glibc's sincos, which differs from sin / cos in the last bit of some
# arguments; the product's host detector (clang) calls sin and cos
EXACT_LIBM = EXACT + ["-fno-builtin"]
WALL = ["-Wall"]
STRICT = ["-Wall", "-Werror"]
# (the two -Wno: pragmas and unused device functions of the EM headers em_plan.hpp includes)
WALL_EM = ["-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function"]
SANITIZED = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

# key -> (source in tests/hostsim, extra flags); the library is libvpk_hostsim_<key>.so but for the two in NAMES
LIBS = {
    "em": ("sim_em.cpp", EXACT_EM),
    "measure": ("sim_em_measure.cpp", EXACT_EM),
    "estep_zeros": ("sim_em_estep_zeros.cpp", EXACT_EM),
    "vpset": ("sim_vpset.cpp", EXACT_EM),
    "emstep": ("sim_emstep.cpp", EXACT_EM),
    "estep": ("sim_estep.cpp", EXACT_EM),
    "overlay": ("sim_overlay.cpp", EXACT_EM),
    "raster": ("sim_raster.cpp", EXACT),
    "lines": ("sim_lines.cpp", EXACT),
    "prior": ("sim_prior.cpp", EXACT),
    "score": ("sim_score.cpp", EXACT),
    "detect": ("sim_detect.cpp", EXACT),
    "train": ("sim_train.cpp", EXACT),
    "convtrain": ("sim_convtrain.cpp", EXACT),
    "trainset": ("sim_trainset.cpp", EXACT),
    "pm": ("pm_driver.cpp", EXACT),
    "lsd": ("sim_lsd.cpp", EXACT_LIBM),
    "frontend": ("sim_frontend.cpp", EXACT_LIBM),
    "train_plan": ("sim_train_plan.cpp", WALL + EXACT),
    "em_plan": ("sim_em_plan.cpp", WALL_EM),
    "batch_args": ("sim_batch_args.cpp", WALL),
    "lsd_plan": ("sim_lsd_plan.cpp", WALL),
    "cnn_plan": ("sim_cnn_plan.cpp", STRICT),
    "cnn_model": ("sim_cnn_model.cpp", STRICT),
}
NAMES = {"em": "libvpk_hostsim.so", "pm": "libvpk_pm.so"}

# program -> (source in tests/hostsim, extra flags)
DRIVERS = {
    "em_plan_driver": ("em_plan_driver.cpp", WALL_EM),
    "train_plan_driver": ("train_plan_driver.cpp", WALL),
    "cnn_model_driver": ("cnn_model_driver.cpp", WALL),
    "lsd_host_driver": ("lsd_host_driver.cpp", EXACT_LIBM),
}


def lib_name(key):
    return NAMES.get(key, "libvpk_hostsim_%s.so" % key)


def _row(key):
    """(source, flags, outdir, name) of a library or a driver: build()'s arguments"""
    if key in LIBS:
        src, extra = LIBS[key]
        return os.path.join(HERE, src), SHARED + extra, BUILD, lib_name(key)
    src, extra = DRIVERS[key]
    return os.path.join(HERE, src), SANITIZED + extra, BUILD, key


class _Job:
    """One product: `name` in `outdir`, from `src` with `flags`, its .d and .stamp beside it.  Everything that is recorded
    or digested is spelled relative to `root`, which is also the directory g++ runs in."""

    def __init__(self, src, flags, outdir, name, root):
        self.root, self.outdir = root, outdir
        self.out = os.path.join(outdir, name)
        self.dep, self.stamp = self.out + ".d", self.out + ".stamp"
        self.src = os.path.relpath(src, root)
        self.flags = list(flags)
        self.tmp = []

    def command(self, out, dep):
        return ["g++"] + self.flags + ["-MMD", "-MF", os.path.relpath(dep, self.root), self.src, "-o",
                                       os.path.relpath(out, self.root)]

    def deps(self):
        """the dependency file's prerequisites inside the repository, normalised and relative to its root"""
        with open(self.dep) as f:
            words = shlex.split(f.read().replace("\\\n", " "))
        inside = {os.path.normpath(w) for w in words[1:]}               # words[0] is the target
        return sorted(d for d in inside if not os.path.isabs(d) and not d.startswith(os.pardir + os.sep))

    def digest(self):
        """None where the dependency file or a file it lists is missing"""
        h = hashlib.sha256(repr(self.command(self.out, self.dep)).encode())
        try:
            for d in self.deps():
                with open(os.path.join(self.root, d), "rb") as f:
                    h.update(("\n%s\n" % d).encode() + hashlib.sha256(f.read()).digest())
        except OSError:
            return None
        return h.hexdigest()

    def fresh(self):
        try:
            with open(self.stamp) as f:
                return os.path.exists(self.out) and f.read() == self.digest()
        except OSError:
            return False

    def start(self):
        os.makedirs(self.outdir, exist_ok=True)
        stem = "%s.%d.tmp" % (self.out, os.getpid())                      # names of this builder alone
        self.tmp = [stem, stem + ".d", stem + ".stamp"]
        return subprocess.Popen(self.command(*self.tmp[:2]), cwd=self.root)

    def finish(self, proc):
        try:
            if proc.wait() != 0:
                raise RuntimeError("g++ failed on " + self.src)
            os.replace(self.tmp[0], self.out)
            os.replace(self.tmp[1], self.dep)
            with open(self.tmp[2], "w") as f:
                f.write(self.digest())
            os.replace(self.tmp[2], self.stamp)                           # the stamp last: without it nothing is fresh
        finally:
            for path in self.tmp:
                if os.path.exists(path):
                    os.remove(path)
            self.tmp = []


def build(src, flags, outdir, name, root=ROOT):
    """`name` in `outdir`, rebuilt from `src` with `flags` if it is stale; returns its path.  Raises if g++ fails, and then
    the previous product, dependency file and stamp are as they were."""
    job = _Job(src, flags, outdir, name, root)
    if not job.fresh():
        job.finish(job.start())
    return job.out


def recorded_deps(key):
    """what g++ reported for a built row, relative to the repository's root"""
    return _Job(*_row(key), ROOT).deps()


_loaded = {}


def load(key):
    """the ctypes.CDLL of a row of LIBS, built first if it is stale; one per process"""
    if key not in _loaded:
        _loaded[key] = ctypes.CDLL(build(*_row(key)))
    return _loaded[key]


def build_all(keys=LIBS):
    """Every stale row of `keys`, at most min(16, cpu count) compilers at a time; raises after the last one if any failed."""
    stale = [j for j in (_Job(*_row(k), ROOT) for k in keys) if not j.fresh()]
    limit, running, failed = min(16, os.cpu_count() or 1), [], []

    def finish_oldest():
        job, proc = running.pop(0)
        try:
            job.finish(proc)
        except RuntimeError as e:
            failed.append(str(e))

    for job in stale:
        if len(running) == limit:
            finish_oldest()
        running.append((job, job.start()))
    while running:
        finish_oldest()
    if failed:
        raise RuntimeError("; ".join(failed))
    return [j.out for j in stale]


def run_drivers():
    build_all(DRIVERS)
    for key in DRIVERS:
        exe = os.path.join(BUILD, key)
        print("$", os.path.relpath(exe, ROOT), flush=True)
        code = subprocess.call([exe])
        if code != 0:
            raise SystemExit("%s exited with %d" % (key, code))


if __name__ == "__main__":
    if sys.argv[1:] == ["drivers"]:
        run_drivers()
    elif not sys.argv[1:]:
        print("\n".join(build_all()))
    else:
        raise SystemExit(__doc__)
