"""Developer tool: compare two device assembly listings kernel by kernel, to show that a change left a kernel's code
alone.  Not part of the product or tests.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -Iinclude --cuda-device-only -S csrc/knn.hip -o before.s   (old source)
    hipcc ... -o after.s                                                                                   (new source)
    python scripts/dev/diff_kernel_isa.py before.s after.s

A file with a ``FLAGS_<file>`` line in csrc/Makefile needs those flags on the hipcc line too: the files that include
pair_walk.hpp do not compile without ``-ffp-contract=off -DCGNN_PAIR_CONTRACT_OFF``.

Compared per function: instructions, labels and directives between the function's label and its end marker.  Dropped
or normalised, because they change when functions are added to a file or a defaulted template argument appears:
comments, the per-function number in ``.LBB<n>_<m>`` labels, and a trailing ``, 0`` integer template argument in the
mangled names (``ILi16ELi0EEE`` is compared with ``ILi16EEE``).  Prints SAME / DIFF / NEW / GONE per function and exits 1
when a function present in both differs."""
import re
import sys


def functions(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        line = line.split(";")[0].rstrip()
        if line:
            out[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", line))
    return out


def plain(name):
    return re.sub(r"ILi(\d+)ELi0EEE", r"ILi\1EEE", name)


def main(before, after):
    a = {plain(k): v for k, v in functions(before).items()}
    b = {plain(k): v for k, v in functions(after).items()}
    differ = 0
    for name in sorted(set(a) | set(b)):
        if name not in a:
            print(f"NEW   {len(b[name]):6d}         {name}")
        elif name not in b:
            print(f"GONE  {len(a[name]):6d}         {name}")
        else:
            same = [plain(x).replace(name, "@") for x in a[name]] == [plain(x).replace(name, "@") for x in b[name]]
            differ += not same
            print(f"{'SAME' if same else 'DIFF'}  {len(a[name]):6d} {len(b[name]):6d}  {name}")
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
