"""The host side of GOP lanes: GOP ranges and a pool that runs whole GOPs on
several host threads and returns the frames in frame order (DESIGN.md "GOP
lanes for sequence files: the host side").

An I frame resets the DPB, every payload carries its own q and ``frame_idx``
and a frame's digest covers only that frame's DPB, so the GOPs of a sequence
file are independent pieces of work.  This module holds what a driver that
codes them at once needs on the host and nothing that touches a GPU:
``gop_ranges`` / ``gops_of`` say which pieces there are (``keyframe_before``:
the piece a frame lies in, where a seek starts decoding), ``LanePool`` hands
them to lanes and keeps the order, the memory bound and the failure rules.
The readers' ``read_frame`` (harness.py) and ``SequenceReader.index()``
(sequence.py) give each lane random access to its frames.

No driver in the package runs codecs on several HIP streams yet:
``encode_video`` / ``decode_video`` stay serial (DESIGN.md says why).
"""
import contextlib
import threading


def gop_ranges(frame_num, gop_size):
    """[(start, stop), ...] of the GOPs of ``frame_num`` frames with an I frame
    every ``gop_size``; the last GOP may be short."""
    if frame_num < 0 or gop_size < 1:
        raise ValueError(f"no GOPs of {gop_size!r} frames in {frame_num!r} frames")
    return [(s, min(s + gop_size, frame_num)) for s in range(0, frame_num, gop_size)]


def gops_of(index, path="the file"):
    """[(start, stop), ...] from the record types of ``SequenceReader.index()``:
    a GOP starts at every I frame, whatever its length."""
    from .sequence import SequenceFormatError
    if index and index[0].type != "I":
        raise SequenceFormatError(f"{path}: frame 0 is a P frame with no frame before it")
    starts = [e.frame_idx for e in index if e.type == "I"]
    return list(zip(starts, starts[1:] + [len(index)]))


def keyframe_before(index, frame_idx, path="the file"):
    """The ``IndexEntry`` of the last I frame at or before ``frame_idx`` in
    ``SequenceReader.index()``: where a decode that wants ``frame_idx`` starts."""
    from .sequence import SequenceFormatError
    if isinstance(frame_idx, bool) or not isinstance(frame_idx, int) or not 0 <= frame_idx < len(index):
        raise ValueError(f"frame {frame_idx!r} is outside 0..{len(index) - 1}")
    if index[0].type != "I":
        raise SequenceFormatError(f"{path}: frame 0 is a P frame with no frame before it")
    k = frame_idx
    while index[k].type != "I":
        k -= 1
    return index[k]


class Lane:
    """What the pool needs of a lane: a number, ``context()`` (a context
    manager the lane's thread runs under) and ``drain()`` (called by that
    thread when it has no more work).  A lane that owns a device stream enters
    it in ``context`` and synchronises it in ``drain``; this one owns nothing."""

    def __init__(self, number):
        self.number = number

    def context(self):
        return contextlib.nullcontext()

    def drain(self):
        pass


class LanePool:
    """Runs ``work(lane, start, stop)`` for every GOP of ``gops`` on the lanes'
    threads (each inside its ``lane.context()``, ``lane.drain()`` at the end).
    ``work`` is a generator function that yields one result per frame of its
    GOP, in order.

    ``run`` is a generator for the calling thread: (frame index, result) in
    frame order.  Lanes take the GOPs in order from one counter, and GOP g is
    begun only once GOP g - lanes has been consumed entirely, so the results
    waiting on the host never exceed ``lanes`` GOPs however long the video is.

    An exception in a lane is kept with the index of the frame it was working
    on.  GOPs that start after that frame stop between frames and no new one
    is begun; GOPs before it run to their end, so ``run`` yields every frame
    before the failing one and then raises its exception, the one of the
    lowest frame when several fail.  An exception outside any frame (from
    ``context`` or ``drain``) is raised once every lane has left and the frame
    the caller waits for has not come, or else after the last frame.  When
    ``run`` ends, for whatever reason (closing the generator included), every
    lane stops between frames and every thread is joined before control
    returns."""

    def __init__(self, lanes):
        self.lanes = list(lanes)

    def run(self, gops, work):
        gops = list(gops)
        cv = threading.Condition()
        results, errors = {}, {}
        st = {"next": 0, "consumed": 0, "fail_at": float("inf"), "abort": False, "broken": None}
        width = len(self.lanes)
        st["alive"] = min(width, len(gops))         # lane threads that may still produce a frame

        def stopped(start):
            return st["abort"] or start > st["fail_at"]

        def take():
            """The next GOP for the calling lane, or None when it is done."""
            with cv:
                while True:
                    g = st["next"]
                    if g >= len(gops) or stopped(gops[g][0]):
                        return None
                    if g < st["consumed"] + width:
                        st["next"] = g + 1
                        return gops[g]
                    cv.wait()

        def lane_main(lane):
            try:
                with lane.context():
                    while True:
                        gop = take()
                        if gop is None:
                            break
                        idx = start = gop[0]
                        try:
                            with contextlib.closing(work(lane, *gop)) as frames:
                                for idx in range(*gop):
                                    with cv:
                                        if stopped(start):
                                            break
                                    res = next(frames)
                                    with cv:
                                        results[idx] = res
                                        cv.notify_all()
                        except BaseException as e:  # noqa: BLE001 - re-raised on the calling thread
                            with cv:
                                errors[idx] = e
                                st["fail_at"] = min(st["fail_at"], idx)
                                cv.notify_all()
                    lane.drain()
            except BaseException as e:  # noqa: BLE001 - re-raised on the calling thread
                with cv:
                    st["broken"] = st["broken"] or e
            finally:
                with cv:
                    st["alive"] -= 1
                    cv.notify_all()

        threads = [threading.Thread(target=lane_main, args=(ln,), name=f"dcvc-lane-{ln.number}")
                   for ln in self.lanes[:len(gops)]]
        for t in threads:
            t.start()
        finished = False
        try:
            for g, gop in enumerate(gops):
                for idx in range(*gop):
                    with cv:
                        while idx not in results and idx not in errors and st["alive"]:
                            cv.wait()
                        if idx in errors:
                            raise errors[idx]
                        if idx not in results:      # every lane has left and nobody produced this frame
                            raise st["broken"] or RuntimeError(f"no lane produced frame {idx}")
                        res = results.pop(idx)
                    yield idx, res
                with cv:
                    st["consumed"] = g + 1
                    cv.notify_all()
            finished = True
        finally:
            with cv:
                st["abort"] = True
                cv.notify_all()
            for t in threads:
                t.join()
        if finished and st["broken"] is not None:   # a lane failed after its last frame (drain, leaving its context)
            raise st["broken"]
