"""A child process on a pipe: the encoder y4m.Writer feeds and the decoder the Predictor's video_decoder knob reads.  Never a shell
and never this process's own program; standard error goes into a temporary file and its last 2000 bytes end the error message."""
import shlex
import subprocess
import tempfile


class Child:
    """`argv` started with `.pipe` as its standard input (feed=True) or its standard output (feed=False), the other one the null
    device.  `what` begins every message: "the video encoder", "'clip.mkv': the video decoder".  A command that cannot be started
    raises RuntimeError.  The caller closes `.pipe` when it is done with it and then calls finish()."""

    def __init__(self, argv, what, feed):
        self.what, self.feed = f"{what} `{' '.join(shlex.quote(a) for a in argv)}`", bool(feed)
        self._err = tempfile.TemporaryFile()
        try:
            self.proc = subprocess.Popen(argv, stdin=subprocess.PIPE if feed else subprocess.DEVNULL,
                                         stdout=subprocess.DEVNULL if feed else subprocess.PIPE, stderr=self._err)
        except OSError as e:
            self._err.close()
            raise RuntimeError(f"{self.what} could not be started: {e}") from e
        self.pipe = self.proc.stdin if feed else self.proc.stdout

    def poll(self):
        return self.proc.poll()

    def finish(self, limit, failure=None, raising=True):
        """Reaps the child -- waits `limit` seconds, then kills it -- and returns its exit status.  With `raising`, a `failure`
        (the caller's words) or a non-zero status raises RuntimeError naming the command, the status, the failure and the tail
        of the child's standard error.  A fed child that had to be killed is a failure."""
        try:
            status = self.proc.wait(timeout=limit)
        except subprocess.TimeoutExpired:
            self.proc.kill()
            status = self.proc.wait()
            if self.feed:
                failure = failure or "it did not end after its standard input was closed"
        self._err.seek(0)
        tail = self._err.read()[-2000:].decode("utf-8", "replace").strip()
        self._err.close()
        if raising and (failure is not None or status != 0):
            raise RuntimeError(f"{self.what} failed with exit status {status}" + (f": {failure}" if failure is not None else "")
                               + (f"; its standard error ends: {tail}" if tail else ""))
        return status
