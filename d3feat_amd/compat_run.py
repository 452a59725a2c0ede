"""Run one of the reference's inference scripts UNCHANGED on the MI355X path:

    python -m d3feat_amd.compat_run /path/to/D3Feat/demo_registration.py
    python -m d3feat_amd.compat_run /path/to/D3Feat/test_3dmatch.py
    python -m d3feat_amd.compat_run /path/to/D3Feat/test_kitti.py
    python -m d3feat_amd.compat_run /path/to/D3Feat/test_eth.py

The script file is executed as it is (runpy, __name__ == '__main__').  What changes is what its imports resolve to: the
repository's compat/ tree is put first on sys.path, so that `tensorflow` / `open3d` (SURVEY.md §8b's symbol list) and the
reference's own package names `utils` / `datasets` / `models` / `kernels` are the d3feat_amd-backed modules -- the script's
directory is NOT on sys.path, the reference's TF-1 implementation is never imported.

Working directory: the scripts read and write paths relative to the checkout (demo_data/*.ply, results/Log_*/..., and they
WRITE demo_data/*.npz / geometric_registration/...).  By default a scratch directory is created that mirrors the checkout's
top level with symlinks (directories that receive outputs are real directories holding symlinks to the inputs), so a
read-only checkout stays untouched; --cwd DIR uses DIR as it is.

Breakpoints: test_eth.py:35-36 stops in pdb.set_trace() before it edits the configuration.  With --skip-breakpoints (the default when
stdin is no terminal; --keep-breakpoints turns it off) pdb.set_trace is, for the run only, a function that prints one line and
returns.  The pdb module itself stays the standard library's; a script that never calls it runs exactly as without the option.
"""
import argparse
import os
import runpy
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPAT = os.path.join(ROOT, "compat")


def _mirror(src_root, dst_root, writable=("demo_data", "geometric_registration", "geometric_registration_kitti", "geometric_registration_eth")):
    os.makedirs(dst_root, exist_ok=True)
    for name in os.listdir(src_root):
        s, d = os.path.join(src_root, name), os.path.join(dst_root, name)
        if os.path.lexists(d):
            continue
        if name in writable and os.path.isdir(s):
            os.makedirs(d)
            for f in os.listdir(s):
                os.symlink(os.path.join(s, f), os.path.join(d, f))
        else:
            os.symlink(s, d)
    for name in writable:
        os.makedirs(os.path.join(dst_root, name), exist_ok=True)


def install_paths():
    """Put compat/ (and the repository) first on sys.path; matplotlib's stand-in only when the real one is missing."""
    for p in (ROOT, COMPAT):
        while p in sys.path:
            sys.path.remove(p)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, COMPAT)
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        sys.path.append(os.path.join(COMPAT, "_optional"))
    for mod in ("tensorflow", "open3d", "utils", "datasets", "models", "kernels"):
        m = sys.modules.get(mod)
        if m is not None and not os.path.abspath(getattr(m, "__file__", "") or "").startswith(COMPAT):
            raise RuntimeError("module %r is already imported from %s: start from a fresh interpreter" % (mod, m.__file__))


def _skipped_breakpoint(*args, **kwargs):
    print("[compat_run] pdb.set_trace() skipped (--skip-breakpoints)")


def run(script, argv=(), cwd=None, allow_missing_checkpoint=False, skip_breakpoints=None):
    """skip_breakpoints: None = when stdin is no terminal."""
    import pdb
    script = os.path.abspath(script)
    if skip_breakpoints is None:
        skip_breakpoints = not (sys.stdin is not None and sys.stdin.isatty())
    if cwd is None:
        cwd = tempfile.mkdtemp(prefix="d3feat_compat_")
        _mirror(os.path.dirname(script), cwd)
    if allow_missing_checkpoint:
        os.environ["D3FEAT_COMPAT_ALLOW_MISSING_CHECKPOINT"] = "1"
    install_paths()
    old_cwd, old_argv, old_trace = os.getcwd(), sys.argv, pdb.set_trace
    os.chdir(cwd)
    sys.argv = [script] + list(argv)
    if skip_breakpoints:
        pdb.set_trace = _skipped_breakpoint
    try:
        return runpy.run_path(script, run_name="__main__"), cwd
    finally:
        pdb.set_trace = old_trace
        os.chdir(old_cwd)
        sys.argv = old_argv


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("script")
    ap.add_argument("--cwd", default=None, help="run in this directory instead of a scratch mirror of the script's checkout")
    ap.add_argument("--allow-missing-checkpoint", action="store_true",
                    help="tf.train.Saver.restore keeps the initial weights when snap-*.data-* is absent (public checkout)")
    ap.add_argument("--skip-breakpoints", dest="skip_breakpoints", action="store_true", default=None,
                    help="pdb.set_trace() prints one line and returns (test_eth.py:35-36); the default when stdin is no terminal")
    ap.add_argument("--keep-breakpoints", dest="skip_breakpoints", action="store_false", help="leave pdb.set_trace() as it is")
    a, rest = ap.parse_known_args()          # anything unknown goes to the script
    _, cwd = run(a.script, rest, a.cwd, a.allow_missing_checkpoint, a.skip_breakpoints)
    print("[compat_run] working directory: %s" % cwd)


if __name__ == "__main__":
    main()
