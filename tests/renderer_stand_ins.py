"""Stand-ins for the CPU-side tests of the Python layer's refusals (test_vertex_update_abi.py, test_skin_abi.py, test_morph_abi.py): a
Renderer without a scene or a library, and a tensor that answers like one on a GPU."""
import torch


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name}): the refusal must come before the call")


def renderer_without_scene(vertices=10, skins=(), morphs=()):
    from vkrt_amd.renderer import Renderer

    r = Renderer.__new__(Renderer)  # no scene: the checks run before any use of the handle
    r.device = 0
    r._vertex_count = vertices
    r._skins = list(skins)
    r._morphs = list(morphs)
    r._h = None
    r.lib = NoLibrary()
    return r


class _Dev:
    def __init__(self, index):
        self.index = index

    def __str__(self):
        return f"cuda:{self.index}"


class Fake(torch.Tensor):
    """answers like a float32 CUDA tensor of the given shape; holds no data"""

    @staticmethod
    def __new__(cls, shape, dtype=torch.float32, index=0, contiguous=True, ptr=0x1000):
        t = torch.Tensor._make_subclass(cls, torch.zeros(shape, dtype=dtype))
        t._index, t._contiguous, t._ptr = index, contiguous, ptr
        return t

    @property
    def is_cuda(self):
        return True

    @property
    def device(self):
        return _Dev(self._index)

    def is_contiguous(self, *a, **k):
        return self._contiguous

    def data_ptr(self):
        return self._ptr
