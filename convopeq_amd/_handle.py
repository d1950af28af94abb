"""What the ctypes wrappers of the objects beside the engine share (cpq_loudness, cpq_limiter, cpq_scorer, cpq_learner; StreamResampler keeps its own copy):
the handle from <prefix>_create, the object's own <prefix>_last_error behind every status, close / __del__ through
<prefix>_destroy, and for the objects that have one, set_stream."""
import ctypes as C

from . import _capi as K
from .engine import CpqError


class Handle:
    _PREFIX = ""            # "cpq_limiter": the C functions of the object are <prefix>_create, _destroy, _last_error ...
    _h = None               # a constructor that raises leaves an object close() accepts

    def _fn(self, name):
        return getattr(self._lib, self._PREFIX + name)

    def _open(self, *args):
        """<prefix>_create(*args, &handle); a refusal raises with the reason the library keeps for calls without an object"""
        self._lib = K.load()
        h = C.c_void_p()
        rc = self._fn("_create")(*args, C.byref(h))
        if rc != K.CPQ_OK:
            raise CpqError(rc, self._fn("_last_error")(None).decode())
        self._h = h

    def _check(self, rc):
        if rc != K.CPQ_OK:
            raise CpqError(rc, self._fn("_last_error")(self._h).decode())

    def close(self):
        if self._h is not None:
            self._fn("_destroy")(self._h)
            self._h = None

    def __del__(self):
        self.close()


class StreamHandle(Handle):
    _stream = None

    def set_stream(self, stream):
        """the torch.cuda.Stream (None: the null stream) later calls enqueue on; the stream used so far is synchronised first"""
        self._check(self._fn("_set_stream")(self._h, C.c_void_p(stream.cuda_stream if stream is not None else None)))
        self._stream = stream           # kept alive as long as the object enqueues on it
