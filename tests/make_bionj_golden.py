"""Regenerate tests/golden/bionj_cases.json (container only, never run by a test): a two-line driver over the reference's
bionj.h is written to a temporary directory, compiled there and run on the fixture matrices of tests/bionj_ref.py.  Each
case holds the matrix as the 7-decimal text the reference reads and the Newick string it wrote.  Neither the driver nor
the binary is kept.
    python tests/make_bionj_golden.py [reference directory, default /root/reference]"""
import json
import os
import subprocess
import sys
import tempfile

import bionj_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
DRIVER = '#include "bionj.h"\nint main(int argc, char **argv) { BioNj b; return argc == 3 ? b.create(argv[1], argv[2]) : 2; }\n'


def cases():
    for n in (5, 8, 13, 24, 40):
        for seed in (0, 1):
            yield "uniform_n%d_s%d" % (n, seed), br.uniform_matrix(n, seed)
    yield "uniform_n65_s1", br.uniform_matrix(65, 1)
    for n in (9, 16):
        yield "duplicates_n%d" % n, br.duplicates_matrix(n)
    yield "balanced_n16_e0.125", br.balanced_matrix(4, 0.125)
    yield "star_n9_d0.5", br.star_matrix(9, 0.5)


def main():
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "driver.cpp"), os.path.join(tmp, "driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call(["g++", "-O2", "-w", "-I", REF, "-o", exe, src])
        for name, D in cases():
            names = ["T%d" % i for i in range(D.shape[0])]
            text = br.matrix_text(D, names)
            fin, fout = os.path.join(tmp, "in.dist"), os.path.join(tmp, "out.nwk")
            with open(fin, "w") as f:
                f.write(text)
            subprocess.check_call([exe, fin, fout], stdout=subprocess.DEVNULL)
            with open(fout) as f:
                newick = f.read().strip()
            out.append(dict(name=name, matrix=text, newick=newick))
    path = os.path.join(ROOT, "tests", "golden", "bionj_cases.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("%d cases, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
