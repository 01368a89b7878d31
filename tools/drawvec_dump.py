"""Writes the cases tools/drawvec_host.cpp walks under a sanitizer: the synthetic tables of the overlay's kernel test
(tests/_drawinfo_cases.py) at every geometry and mode, with the result of the sequential definition (tests/_drawinfo.py).
    python tools/drawvec_dump.py cases.bin
Per case: int32 w, h, blk_w, blk_h, mode, n; n tables of dsv1_blockinfo; n luma planes in; n luma planes as the definition leaves them."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _drawinfo as DI                      # noqa: E402
import _drawinfo_cases as K                 # noqa: E402


def main(path):
    with open(path, "wb") as f:
        for (w, h, bw, bh) in K.KERNEL_GEOMS:
            tabs = K.kernel_tables(w, h, bw, bh)
            n = tabs.shape[0]
            planes = np.random.default_rng(w + h).integers(1, 255, (n, h, w), dtype=np.uint8)
            for mode in range(1, 8):
                want = planes.copy()
                for t in range(n):
                    DI.draw_info(want[t], bw, bh, tabs[t], mode)
                f.write(np.array([w, h, bw, bh, mode, n], dtype="<i4").tobytes())
                f.write(tabs.tobytes())
                f.write(planes.tobytes())
                f.write(want.tobytes())


if __name__ == "__main__":
    main(sys.argv[1])
