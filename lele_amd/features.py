"""lele::features on the device (host mirror of /root/reference/src/features/*.rs)."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from .tensor import TensorView, unwrap


@dataclass
class FeatureConfig:  # pipeline.rs:8-27
    sample_rate: int = 16000
    n_mels: int = 80
    frame_length_ms: float = 25.0
    frame_shift_ms: float = 10.0
    lfr_m: int = 7
    lfr_n: int = 6


def _ctx(ctx):
    from . import default_ctx
    return ctx if ctx is not None else default_ctx()


def _adopt(ctx, obj):
    """obj keeps ctx's stream: ctx.close() closes it first.  Destroying it AFTER its context (an object still alive when the interpreter
    exits, e.g. in the traceback of an uncaught exception) would synchronise a stream that is gone."""
    import weakref
    ctx._children.append(weakref.ref(obj))


class SenseVoiceFrontend:
    """SenseVoiceFrontend (pipeline.rs:28-193): compute(pcm) -> TensorView [T, n_mels*lfr_m]."""

    def __init__(self, config=None, ctx=None):
        self.config = config or FeatureConfig()
        self.ctx = _ctx(ctx)
        c = self.config
        cfg = _lib.LeleFeatureConfig(c.sample_rate, c.n_mels, c.frame_length_ms, c.frame_shift_ms, c.lfr_m, c.lfr_n)
        self._h = C.c_void_p()
        _lib.check(_lib.lib().lele_hip_frontend_create(self.ctx._h, C.byref(cfg), C.byref(self._h)))
        self._out = self.ctx.buf()
        _adopt(self.ctx, self)

    def close(self):
        if self._h:
            _lib.lib().lele_hip_frontend_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def out_rows(self, pcm_len):
        rows, cols, nf = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().lele_hip_frontend_out_rows(self._h, C.c_int64(pcm_len), C.byref(rows), C.byref(cols),
                                                         C.byref(nf)))
        return rows.value, cols.value, nf.value

    def set_profiling(self, on):
        _lib.check(_lib.lib().lele_hip_frontend_set_profiling(self._h, C.c_int(1 if on else 0)))

    def profile_read(self):
        """-> (avg ms of fe_frame_sum_kernel, avg ms of fe_main_kernel, runs)"""
        a, b, n = C.c_float(), C.c_float(), C.c_int64()
        _lib.check(_lib.lib().lele_hip_frontend_profile_read(self._h, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def _call(self, fn, pcm, out):
        keep = []
        t = _lib.as_tensor(unwrap(pcm), keep)
        sh = _lib.OutShape()
        out = out or self._out
        _lib.check(fn(self._h, t, out._h, sh.shape, C.byref(sh.rank)))
        if sh.rank.value == 0:
            return TensorView.empty()  # pcm shorter than one frame (pipeline.rs:70-72)
        return TensorView(_lib.DevTensor(out, sh.get(), np.float32))

    def compute(self, pcm, out=None):
        return self._call(_lib.lib().lele_hip_frontend_compute, pcm, out)

    def compute_batch(self, pcm, out=None):
        """pcm [batch, pcm_len] -> [batch, T, n_mels*lfr_m] (one launch pair for the whole batch)"""
        return self._call(_lib.lib().lele_hip_frontend_compute_batch, pcm, out)

    def compute_segments(self, pcm, segments, out=None):
        """Features of several (start, end) sample ranges of ONE pcm buffer [N] in one launch -- `segments` as apps.vad_segments
        returns them (any order; overlaps and repeats allowed).  -> (TensorView [R, n_mels*lfr_m], offsets np.int64 [count + 1]):
        rows offsets[i] .. offsets[i+1] are compute(pcm[start_i:end_i]), bit for bit (0 rows for a range shorter than one frame)."""
        seg = np.asarray(segments, np.int64).reshape(-1, 2)
        starts = np.ascontiguousarray(seg[:, 0])
        lengths = np.ascontiguousarray(seg[:, 1] - seg[:, 0])
        offsets = np.zeros(len(seg) + 1, np.int64)
        keep = []
        t = _lib.as_tensor(unwrap(pcm), keep)
        sh = _lib.OutShape()
        out = out or self._out
        _lib.check(_lib.lib().lele_hip_frontend_compute_segments(self._h, t, _lib.i64_ptr(starts), _lib.i64_ptr(lengths), len(seg), out._h,
                                                                 _lib.i64_ptr(offsets), sh.shape, C.byref(sh.rank)))
        if sh.rank.value == 0:
            return TensorView.empty(), offsets
        return TensorView(_lib.DevTensor(out, sh.get(), np.float32)), offsets

    def logmel(self, pcm, out=None):
        """intermediate log-mel [num_frames, n_mels] (before LFR); test hook"""
        return self._call(_lib.lib().lele_hip_frontend_logmel, pcm, out)


def stream_rows(config, samples_before, chunk_len, final=False):
    """The closed forms of chunked streaming (lele_hip_frontend_stream_rows; host arithmetic, no GPU): pushing chunk_len samples onto a
    stream that has seen samples_before -> (rows emitted, frames completed, samples carried, log-mel rows carried after the push)."""
    c = config or FeatureConfig()
    cfg = _lib.LeleFeatureConfig(c.sample_rate, c.n_mels, c.frame_length_ms, c.frame_shift_ms, c.lfr_m, c.lfr_n)
    r = [C.c_int64() for _ in range(4)]
    _lib.check(_lib.lib().lele_hip_frontend_stream_rows(C.byref(cfg), C.c_int64(int(samples_before)), C.c_int64(int(chunk_len)),
                                                        C.c_int32(1 if final else 0), *[C.byref(v) for v in r]))
    return tuple(v.value for v in r)


class FrontendStream:
    """`streams` live audio streams fed chunk by chunk through one SenseVoiceFrontend (at most max_chunk samples a stream and push).
    push() returns every feature row that has become final; concatenated per stream the rows are fe.compute(whole utterance), bit for
    bit, for any cut of the audio into chunks (include/lele_hip.h, "chunked streaming")."""

    def __init__(self, fe, streams, max_chunk):
        self.fe, self.streams, self.max_chunk = fe, int(streams), int(max_chunk)
        self._h = C.c_void_p()
        _lib.check(_lib.lib().lele_hip_frontend_stream_create(fe._h, C.c_int64(self.streams), C.c_int64(self.max_chunk), C.byref(self._h)))
        self._out = fe.ctx.buf()
        _adopt(fe.ctx, self)

    def close(self):
        if self._h:
            _lib.lib().lele_hip_frontend_stream_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def push(self, chunks, final=None, out=None):
        """chunks: a list of `streams` 1-D arrays (an empty one: no audio this tick), or (pcm, starts, lengths) with pcm f32 [N] on the
        host or the device and stream i's chunk at pcm[starts[i]:starts[i] + lengths[i]].  final: None or one flag a stream -- the
        utterance of that stream ends with this chunk: its last rows follow (right clamp) and the stream is reset.
        -> (TensorView [R, n_mels*lfr_m], row_offsets np.int64 [streams + 1]): the packed layout of compute_segments."""
        if isinstance(chunks, tuple) and len(chunks) == 3:
            pcm, starts, lengths = chunks
            starts = np.ascontiguousarray(starts, np.int64).reshape(-1)
            lengths = np.ascontiguousarray(lengths, np.int64).reshape(-1)
        else:
            pcm, segs = pack(chunks)
            starts = np.asarray([s for s, _ in segs], np.int64)
            lengths = np.asarray([e - s for s, e in segs], np.int64)
        if len(starts) != self.streams or len(lengths) != self.streams:
            raise _lib.LeleError("FrontendStream.push: %d chunks for %d streams (one entry per stream; an empty chunk for a silent one)"
                                 % (len(starts), self.streams))
        fin = None
        if final is not None:
            fin = np.ascontiguousarray(np.asarray(final).astype(bool), np.uint8).reshape(-1)
            if len(fin) != self.streams:
                raise _lib.LeleError("FrontendStream.push: %d final flags for %d streams" % (len(fin), self.streams))
        offsets = np.zeros(self.streams + 1, np.int64)
        keep = []
        t = _lib.as_tensor(unwrap(pcm), keep)
        sh = _lib.OutShape()
        out = out or self._out
        _lib.check(_lib.lib().lele_hip_frontend_stream_push(
            self._h, t, _lib.i64_ptr(starts), _lib.i64_ptr(lengths), fin.ctypes.data_as(C.POINTER(C.c_uint8)) if fin is not None else None,
            out._h, _lib.i64_ptr(offsets), sh.shape, C.byref(sh.rank)))
        if sh.rank.value == 0:
            return TensorView.empty(), offsets
        return TensorView(_lib.DevTensor(out, sh.get(), np.float32)), offsets

    def reset(self, ids=None):
        """a new utterance in the streams `ids` (None: in all of them); host counters only"""
        if ids is None:
            _lib.check(_lib.lib().lele_hip_frontend_stream_reset(self._h, None, C.c_int64(0)))
        else:
            a = np.ascontiguousarray(ids, np.int64).reshape(-1)
            _lib.check(_lib.lib().lele_hip_frontend_stream_reset(self._h, _lib.i64_ptr(a), C.c_int64(len(a))))

    def _counters(self, k):
        out = np.zeros(self.streams, np.int64)
        v = [C.c_int64(), C.c_int64(), C.c_int64()]
        for i in range(self.streams):
            _lib.check(_lib.lib().lele_hip_frontend_stream_counters(self._h, C.c_int64(i), *[C.byref(x) for x in v]))
            out[i] = v[k].value
        return out

    @property
    def samples_seen(self):
        return self._counters(0)

    @property
    def frames_seen(self):
        return self._counters(1)

    @property
    def rows_emitted(self):
        return self._counters(2)


RESAMPLE_MODES = {"linear": 0, "sinc": 1}


class Resampler:
    """from_rate -> to_rate on the device (include/lele_hip.h, "audio resampling").  mode "linear": the reference's `resample`
    (examples/web-demo/src/audio.rs:114-138) bit for bit; "sinc": a Kaiser-windowed polyphase FIR (z zero crossings a side, beta,
    rolloff).  device=False: a host-only object (out_len, table) that needs no GPU."""

    def __init__(self, from_rate, to_rate, mode="linear", ctx=None, z=16, beta=8.6, rolloff=0.9, device=True):
        if mode not in RESAMPLE_MODES:
            raise _lib.LeleError("Resampler: mode %r is neither 'linear' nor 'sinc'" % (mode,))
        self.from_rate, self.to_rate, self.mode = int(from_rate), int(to_rate), mode
        self.ctx = _ctx(ctx) if device else None
        self._h = C.c_void_p()
        _lib.check(_lib.lib().lele_hip_resampler_create(self.ctx._h if device else None, C.c_int64(self.from_rate), C.c_int64(self.to_rate),
                                                        C.c_int32(RESAMPLE_MODES[mode]), C.c_int32(int(z)), C.c_double(beta), C.c_double(rolloff),
                                                        C.byref(self._h)))
        self._out = self.ctx.buf() if device else None
        if device:
            _adopt(self.ctx, self)

    def close(self):
        if self._h:
            _lib.lib().lele_hip_resampler_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def out_len(self, n, samples_before=0, final=True, with_carry=False):
        """outputs that become final when n samples follow samples_before (lele_hip_resampler_out_len; host arithmetic, no GPU);
        the defaults give the length of a whole utterance's result.  with_carry: -> (outputs, input samples carried afterwards)"""
        o, c = C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().lele_hip_resampler_out_len(self._h, C.c_int64(int(samples_before)), C.c_int64(int(n)), C.c_int32(1 if final else 0),
                                                         C.byref(o), C.byref(c)))
        return (o.value, c.value) if with_carry else o.value

    def table(self):
        """-> (f32 table [L, T] as uploaded, L, M); "linear" has none: shape (1, 0)"""
        l, m, t = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().lele_hip_resampler_table(self._h, None, C.c_int64(0), C.byref(l), C.byref(m), C.byref(t)))
        tab = np.zeros((l.value, t.value), np.float32)
        _lib.check(_lib.lib().lele_hip_resampler_table(self._h, tab.ctypes.data_as(C.c_void_p), C.c_int64(tab.size), None, None, None))
        return tab, l.value, m.value

    def compute_segments(self, pcm, segments, out=None):
        """The (start, end) ranges of ONE pcm buffer [N], each resampled on its own, in one launch.  -> (TensorView [N'], segments'
        np.int64 [count, 2]): range i of the result is the resampled range i -- what SenseVoiceFrontend.compute_segments takes."""
        seg = np.asarray(segments, np.int64).reshape(-1, 2)
        starts = np.ascontiguousarray(seg[:, 0])
        lengths = np.ascontiguousarray(seg[:, 1] - seg[:, 0])
        offsets = np.zeros(len(seg) + 1, np.int64)
        keep = []
        t = _lib.as_tensor(unwrap(pcm), keep)
        sh = _lib.OutShape()
        out = out or self._out
        _lib.check(_lib.lib().lele_hip_resample_segments(self._h, t, _lib.i64_ptr(starts), _lib.i64_ptr(lengths), len(seg), out._h,
                                                         _lib.i64_ptr(offsets), sh.shape, C.byref(sh.rank)))
        segs = np.stack([offsets[:-1], offsets[1:]], axis=1)
        if sh.rank.value == 0:
            return TensorView(np.zeros(0, np.float32)), segs
        return TensorView(_lib.DevTensor(out, sh.get(), np.float32)), segs


class ResamplerStream:
    """`streams` live streams through one Resampler, at most max_chunk input samples a stream and push.  push() returns every output
    sample that has become final; concatenated per stream they are rs.compute_segments on the whole utterance, bit for bit, for any
    cut into chunks."""

    def __init__(self, rs, streams, max_chunk):
        self.rs, self.streams, self.max_chunk = rs, int(streams), int(max_chunk)
        self._h = C.c_void_p()
        _lib.check(_lib.lib().lele_hip_resampler_stream_create(rs._h, C.c_int64(self.streams), C.c_int64(self.max_chunk), C.byref(self._h)))
        self._out = rs.ctx.buf()
        _adopt(rs.ctx, self)

    def close(self):
        if self._h:
            _lib.lib().lele_hip_resampler_stream_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def push(self, chunks, final=None, out=None):
        """chunks and final as FrontendStream.push takes them.  -> (TensorView [N'], starts, lengths): stream i's new samples are
        [starts[i], starts[i] + lengths[i]) of the result -- the tuple FrontendStream.push takes."""
        if isinstance(chunks, tuple) and len(chunks) == 3:
            pcm, starts, lengths = chunks
            starts = np.ascontiguousarray(starts, np.int64).reshape(-1)
            lengths = np.ascontiguousarray(lengths, np.int64).reshape(-1)
        else:
            pcm, segs = pack(chunks)
            starts = np.asarray([s for s, _ in segs], np.int64)
            lengths = np.asarray([e - s for s, e in segs], np.int64)
        if len(starts) != self.streams or len(lengths) != self.streams:
            raise _lib.LeleError("ResamplerStream.push: %d chunks for %d streams (one entry per stream; an empty chunk for a silent one)"
                                 % (len(starts), self.streams))
        fin = None
        if final is not None:
            fin = np.ascontiguousarray(np.asarray(final).astype(bool), np.uint8).reshape(-1)
            if len(fin) != self.streams:
                raise _lib.LeleError("ResamplerStream.push: %d final flags for %d streams" % (len(fin), self.streams))
        offsets = np.zeros(self.streams + 1, np.int64)
        keep = []
        t = _lib.as_tensor(unwrap(pcm), keep)
        sh = _lib.OutShape()
        out = out or self._out
        _lib.check(_lib.lib().lele_hip_resampler_stream_push(
            self._h, t, _lib.i64_ptr(starts), _lib.i64_ptr(lengths), fin.ctypes.data_as(C.POINTER(C.c_uint8)) if fin is not None else None,
            out._h, _lib.i64_ptr(offsets), sh.shape, C.byref(sh.rank)))
        o_starts, o_lengths = offsets[:-1].copy(), np.diff(offsets)
        if sh.rank.value == 0:
            return TensorView(np.zeros(0, np.float32)), o_starts, o_lengths
        return TensorView(_lib.DevTensor(out, sh.get(), np.float32)), o_starts, o_lengths

    def reset(self, ids=None):
        """a new utterance in the streams `ids` (None: in all of them); host counters only"""
        if ids is None:
            _lib.check(_lib.lib().lele_hip_resampler_stream_reset(self._h, None, C.c_int64(0)))
        else:
            a = np.ascontiguousarray(ids, np.int64).reshape(-1)
            _lib.check(_lib.lib().lele_hip_resampler_stream_reset(self._h, _lib.i64_ptr(a), C.c_int64(len(a))))

    def counters(self, i):
        """(samples received, outputs emitted, samples carried) of stream i since its last reset or final push"""
        v = [C.c_int64(), C.c_int64(), C.c_int64()]
        _lib.check(_lib.lib().lele_hip_resampler_stream_counters(self._h, C.c_int64(int(i)), *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)


def pack(arrays):
    """list of 1-D PCM arrays -> (pcm f32 [sum of lengths], [(start, end)]): one buffer for compute_segments"""
    arrays = [np.asarray(a, np.float32).reshape(-1) for a in arrays]
    ends = np.cumsum([len(a) for a in arrays], dtype=np.int64)
    starts = ends - np.asarray([len(a) for a in arrays], np.int64)
    pcm = np.concatenate(arrays) if arrays else np.zeros(0, np.float32)
    return pcm, [(int(s), int(e)) for s, e in zip(starts, ends)]


def _op(ctx, fn, tensors, extra, out=None, dtype=np.float32, prefix=()):
    ctx = _ctx(ctx)
    keep = []
    args = [ctx._h] + list(prefix)
    for t in tensors:
        args.append(_lib.as_tensor(unwrap(t), keep))
    args.extend(extra)
    out = out or ctx.buf()
    sh = _lib.OutShape()
    args.extend([out._h, sh.shape, C.byref(sh.rank)])
    _lib.check(fn(*args))
    return TensorView(_lib.DevTensor(out, sh.get(), dtype))


class Lfr:  # lfr.rs
    def __init__(self, m=7, n=6, ctx=None):
        self.m, self.n, self.ctx = m, n, ctx

    def compute(self, x, out=None):
        return _op(self.ctx, _lib.lib().lele_hip_lfr, [x], [C.c_int64(self.m), C.c_int64(self.n)], out)


class Cmvn:  # cmvn.rs
    def __init__(self, eps=1e-5, ctx=None):
        self.eps, self.ctx = eps, ctx

    def compute(self, x, out=None):
        return _op(self.ctx, _lib.lib().lele_hip_cmvn, [x], [C.c_float(self.eps)], out)

    def compute_segments(self, x, offsets, out=None):
        """x [R, D] packed as compute_segments returns it, offsets [count + 1]: each segment normalised with its own statistics (bit
        for bit compute() on its rows alone; 0-row segments are skipped)"""
        off = np.ascontiguousarray(offsets, np.int64)
        if int(off[-1]) == 0:
            return TensorView.empty()
        return _op(self.ctx, _lib.lib().lele_hip_cmvn_segments, [x], [_lib.i64_ptr(off), C.c_int64(len(off) - 1), C.c_float(self.eps)],
                   out)

    def apply_with_stats(self, x, mean, std, out=None):
        ctx = _ctx(self.ctx)
        keep = []
        out = out or ctx.buf()
        sh = _lib.OutShape()
        _lib.check(_lib.lib().lele_hip_cmvn_apply_with_stats(
            ctx._h, _lib.as_tensor(unwrap(x), keep), _lib.as_tensor(unwrap(mean), keep),
            _lib.as_tensor(unwrap(std), keep), C.c_float(self.eps), out._h, sh.shape, C.byref(sh.rank)))
        return TensorView(_lib.DevTensor(out, sh.get(), np.float32))


class RealFft:  # features/fft.rs:1-49
    def __init__(self, length, ctx=None):
        self.n, self.ctx = length, ctx

    def process(self, x):
        """x [rows, n] or [n] real -> (re, im) each [rows, n/2+1]; n must be the length this RealFft was made for (the assert_eq of fft.rs:24)"""
        a = np.asarray(unwrap(x), np.float32) if not isinstance(unwrap(x), _lib.DevTensor) else unwrap(x)
        last = a.shape[-1] if len(a.shape) else 1
        if last != self.n:
            raise _lib.LeleError("RealFft(%d).process: the input's last dimension is %d, not %d" % (self.n, last, self.n))
        ctx = _ctx(self.ctx)
        keep = []
        if isinstance(a, np.ndarray) and a.ndim == 1:
            a = a.reshape(1, -1)
        o_re, o_im = ctx.buf(), ctx.buf()
        sh = _lib.OutShape()
        _lib.check(_lib.lib().lele_hip_rfft(ctx._h, _lib.as_tensor(a, keep), o_re._h, o_im._h, sh.shape,
                                            C.byref(sh.rank)))
        return (TensorView(_lib.DevTensor(o_re, sh.get(), np.float32)),
                TensorView(_lib.DevTensor(o_im, sh.get(), np.float32)))
