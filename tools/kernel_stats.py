"""The kernels' own times of one run, for the *_profile.py tools' --kernel-stats forms: the script is started as a fresh child process under
`rocprofv3 --kernel-trace --stats` (the program after `--`, no counters in that run), and the rows of the named kernels are kept."""
import csv, glob, os, shutil, subprocess, sys, tempfile


def child_rows(script, child_args, keep, cwd, prefix, timeout=None):
    """(header, rows) of rocprofv3's kernel statistics of `python script child_args...`: the rows whose kernel name keep(name) accepts.  timeout: seconds the
    child may take (subprocess.TimeoutExpired ends the whole tool: nothing more is started after a child that hung)"""
    tmp = tempfile.mkdtemp(prefix=prefix)
    try:
        subprocess.check_call(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(script)]
                              + [str(x) for x in child_args], cwd=cwd, timeout=timeout)
        found = sorted(glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True))
        if not found:
            raise SystemExit("rocprofv3 wrote no kernel statistics under " + tmp)
        table = list(csv.reader(open(found[0])))
        return table[0], [r for r in table[1:] if keep(r[0])]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def write(path, header, rows):
    with open(path, "w", newline="") as f:
        csv.writer(f).writerows([header] + rows)
