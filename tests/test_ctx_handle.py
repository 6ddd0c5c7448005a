"""CPU: there is one ctypes handle of a resident context and one loop over row windows (malstroem_amd/_ctx.py, pipeline.py) -- the
pipeline and the band backend inherit the transfers and getters, and the streaming methods hand their rows to `write_windows`."""
import ast
import inspect
import textwrap

import numpy as np

from malstroem_amd import pipeline
from malstroem_amd._ctx import CtxHandle
from malstroem_amd.distributed import HipBand
from malstroem_amd.pipeline import HydroPipeline


def test_pipeline_and_band_share_the_handle():
    for cls in (HydroPipeline, HipBand):
        assert issubclass(cls, CtxHandle)
        for method in ("upload", "download", "get_int", "close", "__del__"):
            assert method not in vars(cls), (cls.__name__, method)
            assert getattr(cls, method) is getattr(CtxHandle, method)
    # the band's answer to a window of no rows is an override, the pipeline hands such a window to the library
    assert "download_rows" in vars(HipBand) and "download_rows" not in vars(HydroPipeline)


def test_streaming_methods_hold_no_loop_of_their_own():
    for method in ("download_to", "download_wet_at_to", "download_flow_distance_to"):
        src = inspect.getsource(getattr(HydroPipeline, method))
        # (the docstrings say "as ``download_to`` does for the rasters": the statements are what must hold no `for `)
        nodes = list(ast.walk(ast.parse(textwrap.dedent(src))))
        assert not [n for n in nodes if isinstance(n, (ast.For, ast.While, ast.comprehension))], method
        assert "for " not in src.replace(inspect.getdoc(getattr(HydroPipeline, method)), "") and "write_windows(" in src, method
    assert inspect.getsource(pipeline).count("for row0 in range(") == 1


def test_write_windows_partial_last_window_and_fall_back():
    a = np.arange(35, dtype=np.float64).reshape(5, 7)
    calls = []

    def rows(row0, nrows):
        calls.append((row0, nrows))
        return a[row0:row0 + nrows]

    class Windows(object):
        log = []

        def open(self, shape, dtype):
            self.log.append(("open", shape, dtype))

        def write_window(self, row0, array):
            self.log.append((row0, array.copy()))

        def close(self):
            self.log.append("close")

    class Whole(object):
        def write(self, array):
            self.array = array

    w = Windows()
    pipeline.write_windows(w, a.shape, np.float64, rows, 2)
    assert calls == [(0, 2), (2, 2), (4, 1)]
    assert w.log[0] == ("open", (5, 7), np.float64) and w.log[-1] == "close"
    assert [r for r, _ in w.log[1:-1]] == [0, 2, 4] and np.array_equal(np.concatenate([x for _, x in w.log[1:-1]]), a)
    del calls[:]
    whole = Whole()
    pipeline.write_windows(whole, a.shape, np.float64, rows, 2)
    assert calls == [(0, 5)] and np.array_equal(whole.array, a)
