"""Records tests/golden/drawinfo.json: the sha256 of what the reference CLI (oracle/_ref/dsv1) writes for `d -drawinfo7` of each stream
fixture of tests/_drawinfo_cases.py, so that the GPU tests need no compiled reference.
    python tools/make_drawinfo_goldens.py"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _cabi as A                           # noqa: E402
import _drawinfo_cases as K                 # noqa: E402


def main():
    assert os.path.exists(A.REF_CLI), "needs the compiled reference (oracle/_ref)"
    out = {}
    for name, (w, h, seed) in K.STREAMS.items():
        with tempfile.TemporaryDirectory() as td:
            A.ref_cli_encode(K.stream_clip(name), w, h, A.FMT_CLI[A.SUBSAMP_420], K.CLI, td)
            yuv = os.path.join(td, "dec.yuv")
            subprocess.run([A.REF_CLI, "d", "-y", "-inp_" + os.path.join(td, "out.dsv"), "-out_" + yuv, "-drawinfo7"], check=True,
                           stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            with open(yuv, "rb") as f:
                out[name] = hashlib.sha256(f.read()).hexdigest()
    with open(K.GOLDEN, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", K.GOLDEN)


if __name__ == "__main__":
    main()
