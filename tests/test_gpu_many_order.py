"""align_many: which class a job runs in does not depend on where the job stands in the call (csrc/rv_many.hip many_classes, many_class_admits).  The two
mixed batches of the suite -- every class of the built-in picker, every class under the reference's default picker -- run twice on one Batch with every
class threshold at 1: as given, and in reversed order.  A job's result is its set of anchors and its final text, as everywhere in the suite: the order
in which the kernels of a round emit the anchors of one job varies between two runs of the same call.  (An exact comparison of the lists fails at this
commit and at its parent alike: 2 of the 61 jobs of the picker batch, the same anchors in another order, also between a call and its repetition.)"""
import pytest

import many_chain_wide_large_cases as cw
from helpers import oracle  # noqa: F401  (puts the repository root on sys.path)
from reveal_amd import many
from test_gpu_many_chain_wide_large import EVERY_SWITCH, mixed_batch
from test_gpu_many_wide import MINL, every_switch_jobs

pytestmark = pytest.mark.gpu

THRESHOLDS = ("RV_MANY_LARGE_MIN", "RV_MANY_LARGE_MULTI_MIN", "RV_MANY_WIDE_LARGE_MIN", "RV_MANY_CHAIN_LARGE_MIN", "RV_MANY_CHAIN_LARGE_MULTI_MIN",
              "RV_MANY_CHAIN_WIDE_LARGE_MIN")


def built_in():
    return every_switch_jobs(), dict(minlength=MINL, minn=2, toupper=False, multi=True, large=True, large_multi=True, wide=True)


def picker():
    batch, _, _ = mixed_batch([list(fam) for _, fam in cw.jobs()], cw.load_golden())
    return batch, dict(minlength=20, picker=cw.picker_args(dict(minlength=20)), **EVERY_SWITCH)


@pytest.mark.parametrize("make", [built_in, picker])
def test_a_reversed_call_gives_the_same_results_and_the_same_info(make):
    jobs, kw = make()
    b = many.Batch(False)
    for name in THRESHOLDS:
        b.option(name, 1)
    first, info = many.align_many(jobs, batch=b, **kw)
    second, info_reversed = many.align_many(jobs[::-1], batch=b, **kw)
    print("info", info, "reversed", info_reversed)
    del info["stats"], info_reversed["stats"]      # (the counters of rv_many_info are compared; the statistics hold times)
    assert info["rounds"] == 6 and info["ordinary"] == 1
    differ = [j for j, (x, y) in enumerate(zip(first, second[::-1])) if sorted(x["anchors"]) != sorted(y["anchors"]) or x["T"] != y["T"]]
    assert not differ, "%d jobs differ between the two orders, first: job %d of %d sequences" % (len(differ), differ[0], len(jobs[differ[0]]))
    assert info == info_reversed
