"""Child process of tests/test_detect_domain_gpu.py: the detector's dynamic LDS limit (hipFuncAttributeMaxDynamicSharedMemorySize) belongs to the
process, and once a large grid has raised it every smaller grid launches under it.  Whether detect.hip raises it at the FIRST grid that
needs more than 48 KiB (91 x 91: 49,696 B) therefore shows only where no larger grid ran before: in a fresh process (pattern:
tests/multi_prefilter_child.py).  Runs the named cases of tests/detect_cases.py in the order given and prints one JSON object per case:
outcome, area, side and the field as uint32 bit patterns."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(names):
    import detect_cases as dc
    from ofps_amd.runtime import HipContext
    ctx = HipContext(0)
    try:
        for name in names:
            c = dc.BY_NAME[name]
            r = ctx.detect(c.make(), **c.params)
            field = np.zeros((c.side, c.side, 2), np.float32) if r is None else r[1]
            print(json.dumps(dict(name=name, has=r is not None, area=0 if r is None else r[0], side=int(field.shape[0]),
                                  field=np.ascontiguousarray(field).view(np.uint32).reshape(-1).tolist())), flush=True)
    finally:
        ctx.close()


if __name__ == "__main__":
    main(sys.argv[1:])
