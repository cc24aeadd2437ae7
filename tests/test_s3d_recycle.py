"""modelx-s3d recycles deleted data files: a PUT of the same size class
overwrites a pooled file's pages instead of allocating new ones. These tests
hold the pool to what it must never change: every object reads back as its
own bytes at its own length, a GET in flight is never handed another object's
bytes, and the pool stays inside its cap, out of listings, and empty after a
restart.

MODELX_TEST_S3D names another s3d binary to run them against (the sanitizer
builds, `make servers-asan servers-tsan`)."""
import base64
import os
import re
import socket
import threading
import time

import pytest
import requests

from test_crc32c import ref_crc32c
from util_servers import BUCKET, S3D, ServerProc, _build_servers, free_port, wait_http

MIN_BYTES = 16384  # --recycle-min-bytes for these tests (the server's floor is 8 KiB)
KIB = 1024


class Store:
    def __init__(self, root, *flags):
        _build_servers()
        self.root = str(root)
        self.flags = flags
        self.start()

    def start(self):
        port = free_port()
        binary = os.environ.get("MODELX_TEST_S3D", S3D)
        self.srv = ServerProc([binary, "--listen", f"127.0.0.1:{port}", "--root", self.root,
                               "--no-auth", "--recycle-min-bytes", str(MIN_BYTES), *self.flags],
                              port)
        wait_http(port, timeout=30)
        os.makedirs(os.path.join(self.root, BUCKET), exist_ok=True)
        self.base = f"{self.srv.url}/{BUCKET}"
        # one keep-alive connection: s3d counts a file as being read until
        # the connection that got it sends its next request
        self.http = requests.Session()

    def stop(self):
        self.http.close()
        self.srv.stop()

    def metrics(self):
        text = self.http.get(f"{self.srv.url}/.metrics").text
        return {k: float(v) for k, v in (ln.split() for ln in text.splitlines())}

    def wait_for(self, cond):
        """The trash collector works behind the DELETE's 204: poll its counters."""
        deadline = time.monotonic() + 10
        while time.monotonic() < deadline:
            m = self.metrics()
            if cond(m):
                return m
            time.sleep(0.005)
        raise AssertionError(f"collector never got there: {self.metrics()}")

    def put(self, key, data, **kw):
        return self.http.put(f"{self.base}/{key}", data=data, **kw)

    def get(self, key, **kw):
        return self.http.get(f"{self.base}/{key}", **kw)

    def delete(self, key):
        assert self.http.delete(f"{self.base}/{key}").status_code == 204

    def delete_pooled(self, key, n=1):
        """DELETE and wait until the collector has pooled n more files."""
        before = self.metrics()["s3d_recycle_pooled_total"]
        self.delete(key)
        self.wait_for(lambda m: m["s3d_recycle_pooled_total"] == before + n)

    def recycle_files(self):
        d = os.path.join(self.root, ".recycle")
        return [os.path.join(d, n) for n in os.listdir(d)]

    def tmp_files(self):
        return [n for _, _, names in os.walk(self.root) for n in names if ".tmp" in n]


@pytest.fixture
def store(tmp_path):
    s = Store(tmp_path / "s3")
    yield s
    s.stop()


def pattern(n, tag):
    """n bytes that differ between tags at every position."""
    unit = bytes((tag * 37 + i) % 251 for i in range(251))
    return (unit * (n // 251 + 1))[:n]


def test_same_size_put_reuses_deleted_file(store):
    a, b = pattern(256 * KIB, 1), pattern(256 * KIB, 2)
    assert store.put("a", a).status_code == 200
    store.delete_pooled("a")
    assert store.get("a").status_code == 404
    # pooled bytes are no object: not in the listing, not reachable by name
    assert "<Key>" not in requests.get(store.base).text
    (pooled,) = store.recycle_files()
    assert requests.get(f"{store.srv.url}/.recycle/{os.path.basename(pooled)}").status_code == 404
    assert store.put("b", b).status_code == 200
    r = store.get("b")
    assert r.status_code == 200 and int(r.headers["Content-Length"]) == len(b)
    assert r.content == b
    m = store.metrics()
    assert m["s3d_recycle_hits_total"] == 1
    assert m["s3d_recycle_pool_files"] == 0 and m["s3d_recycle_pool_bytes"] == 0
    assert store.recycle_files() == [] and store.tmp_files() == []


def test_smaller_object_in_larger_file_has_no_stale_tail(store):
    big, small = pattern(100000, 3), pattern(90000, 4)
    store.put("big", big)
    store.delete_pooled("big")
    assert store.put("small", small).status_code == 200
    assert store.metrics()["s3d_recycle_hits_total"] == 1
    assert os.path.getsize(os.path.join(store.root, BUCKET, "small")) == len(small)
    r = store.get("small")
    assert int(r.headers["Content-Length"]) == len(small) and r.content == small
    r = store.get("small", headers={"Range": "bytes=89990-89999"})
    assert r.status_code == 206 and r.content == small[-10:]
    r = store.get("small", headers={"Range": "bytes=89990-"})
    assert r.status_code == 206 and r.content == small[-10:]
    assert store.get("small", headers={"Range": "bytes=90000-"}).status_code == 416


def test_sizes_outside_the_class_take_the_plain_path(store):
    store.put("seed", pattern(100000, 5))
    store.delete_pooled("seed")
    cases = {"larger": pattern(200000, 6),        # nothing pooled is that long
             "much-smaller": pattern(50000, 7),   # 100000 > 50000 * 1.25
             "below-min": pattern(MIN_BYTES - 1, 8)}
    for key, data in cases.items():
        assert store.put(key, data).status_code == 200
        r = store.get(key)
        assert int(r.headers["Content-Length"]) == len(data) and r.content == data
    m = store.metrics()
    assert m["s3d_recycle_hits_total"] == 0 and m["s3d_recycle_pool_files"] == 1
    # and a deleted file below the minimum is not pooled
    unlinked = m["s3d_trash_unlinked_total"]
    store.delete("below-min")
    m = store.wait_for(lambda m: m["s3d_trash_unlinked_total"] == unlinked + 1)
    assert m["s3d_recycle_pool_files"] == 1


def test_multipart_parts_in_recycled_files(store):
    part = 64 * KIB
    for i in range(2):
        store.put(f"seed{i}", pattern(part, 10 + i))
        store.delete_pooled(f"seed{i}")
    parts = [pattern(part, 20), pattern(part, 21), pattern(10000, 22)]
    r = requests.post(f"{store.base}/mp?uploads")
    upload_id = re.search(r"<UploadId>(\w+)</UploadId>", r.text).group(1)
    for n, data in enumerate(parts, 1):
        r = requests.put(f"{store.base}/mp?partNumber={n}&uploadId={upload_id}", data=data)
        assert r.status_code == 200
    assert store.metrics()["s3d_recycle_hits_total"] == 2
    assert requests.post(f"{store.base}/mp?uploadId={upload_id}", data="<x/>").status_code == 200
    whole = b"".join(parts)
    r = store.get("mp")
    assert int(r.headers["Content-Length"]) == len(whole) and r.content == whole
    r = store.get("mp", headers={"Range": f"bytes={part - 100}-{2 * part + 99}"})
    assert r.status_code == 206 and r.content == whole[part - 100:2 * part + 100]
    # deleting the object pools its two full-size parts; the short one is unlinked
    store.delete_pooled("mp", n=2)
    assert store.metrics()["s3d_recycle_pool_bytes"] == 2 * part
    assert "<Key>" not in requests.get(store.base).text


def crc_header(data, flip=0):
    return {"x-amz-checksum-crc32c":
            base64.b64encode((ref_crc32c(data) ^ flip).to_bytes(4, "big")).decode()}


def test_checksummed_put_into_recycled_file(store):
    n = 128 * KIB
    store.put("seed", pattern(n + 1000, 30))
    store.delete_pooled("seed")
    good = pattern(n, 31)
    r = store.put("good", good, headers=crc_header(good))
    assert r.status_code == 200 and r.headers["x-amz-checksum-crc32c"]
    assert store.metrics()["s3d_recycle_hits_total"] == 1
    r = store.get("good")
    assert int(r.headers["Content-Length"]) == n and r.content == good
    store.delete_pooled("good")
    bad = pattern(n, 32)
    r = store.put("bad", bad, headers=crc_header(bad, flip=1))
    assert r.status_code == 400 and "BadDigest" in r.text
    assert store.metrics()["s3d_recycle_hits_total"] == 2  # it did write into a pooled file
    assert store.tmp_files() == []
    assert store.get("bad").status_code == 404
    assert store.recycle_files() == []


def test_get_in_flight_never_sees_the_next_objects_bytes(store):
    """A GET holds A open while A is deleted and an equal-sized B is stored.
    The reader's bytes are A's, all of them or a short close; never B's."""
    n = 16 << 20  # several times what the socket buffers below can hold
    a, b = pattern(n, 40), pattern(n, 41)
    store.put("a", a)
    sock = socket.socket()
    sock.setsockopt(socket.SOL_SOCKET, socket.SO_RCVBUF, 64 * KIB)
    sock.connect(("127.0.0.1", store.srv.port))
    sock.settimeout(20)
    sock.sendall(f"GET /{BUCKET}/a HTTP/1.1\r\nHost: x\r\nConnection: close\r\n\r\n".encode())
    got = b""
    while b"\r\n\r\n" not in got:
        got += sock.recv(4096)
    head, body = got.split(b"\r\n\r\n", 1)
    assert b" 200 " in head.split(b"\r\n")[0]
    # the server is now blocked in sendfile with A open
    store.delete("a")
    store.wait_for(lambda m: m["s3d_recycle_busy_total"] == 1)  # seen, and refused
    assert store.recycle_files() == []
    assert store.put("b", b).status_code == 200
    assert store.get("b").content == b
    chunks = [body]
    while True:
        chunk = sock.recv(1 << 20)
        if not chunk:
            break
        chunks.append(chunk)
    sock.close()
    body = b"".join(chunks)
    assert len(body) <= n
    assert body == a[:len(body)]
    # with nobody reading it any more, the same file is pooled
    store.delete_pooled("b")


def upload_multipart(store, key, parts):
    r = requests.post(f"{store.base}/{key}?uploads")
    upload_id = re.search(r"<UploadId>(\w+)</UploadId>", r.text).group(1)
    for n, data in enumerate(parts, 1):
        r = requests.put(f"{store.base}/{key}?partNumber={n}&uploadId={upload_id}", data=data)
        assert r.status_code == 200
    r = requests.post(f"{store.base}/{key}?uploadId={upload_id}", data="<x/>")
    assert r.status_code == 200


def read_until_closed_or(sock, want):
    """What is left of a response body: `want` bytes, or fewer if the
    connection closes first."""
    chunks, got = [], 0
    while got < want:
        chunk = sock.recv(min(1 << 20, want - got))
        if not chunk:
            break
        chunks.append(chunk)
        got += len(chunk)
    return b"".join(chunks)


@pytest.mark.parametrize("close", [False, True], ids=["keep-alive", "connection-close"])
@pytest.mark.parametrize("multipart", [False, True], ids=["object", "multipart"])
@pytest.mark.parametrize("n", [64 * KIB, 1 << 20], ids=["64K", "1M"])
def test_response_left_in_the_socket_buffers_stays_the_old_objects(store, n, multipart, close):
    """The whole response fits the socket buffers, so the server is done with
    it (sendfile returned, and with Connection: close the socket is closed)
    while the client has read the head only. sendfile is zero-copy: what the
    client has not read is still the file's pages. DELETE A and PUT equal-sized
    objects: the rest of the response is A's bytes (or the connection closes
    short), so A's files must not have been recycled under it."""
    parts = [pattern(n, 60), pattern(n, 61)] if multipart else [pattern(n, 60)]
    a = b"".join(parts)
    if multipart:
        upload_multipart(store, "a", parts)
    else:
        store.put("a", a)
    sock = socket.socket()
    sock.connect(("127.0.0.1", store.srv.port))
    sock.settimeout(20)
    extra = "Connection: close\r\n" if close else ""
    sock.sendall(f"GET /{BUCKET}/a HTTP/1.1\r\nHost: x\r\n{extra}\r\n".encode())
    got = b""
    while b"\r\n\r\n" not in got:
        got += sock.recv(256)
    head, body = got.split(b"\r\n\r\n", 1)
    assert b" 200 " in head.split(b"\r\n")[0] and f"Content-Length: {len(a)}".encode() in head
    store.delete("a")
    m = store.wait_for(lambda m: m["s3d_recycle_busy_total"] + m["s3d_recycle_pooled_total"]
                       == len(parts))
    assert m["s3d_recycle_pooled_total"] == 0 and store.recycle_files() == []
    for i in range(len(parts)):
        b = pattern(n, 70 + i)
        assert store.put(f"b{i}", b).status_code == 200
        assert store.get(f"b{i}").content == b
    assert store.metrics()["s3d_recycle_hits_total"] == 0
    body += read_until_closed_or(sock, len(a) - len(body))
    assert body == a[:len(body)]
    sock.close()


def test_reader_count_drops_with_the_connections_next_request(store):
    """A file stays counted as being read until the connection that got it
    asks for something else; a connection that just ends leaves it counted."""
    data = pattern(256 * KIB, 80)
    other = requests.Session()
    for key in ("stays", "drops"):
        store.put(key, data)
        assert other.get(f"{store.base}/{key}").content == data
        if key == "drops":
            assert other.get(f"{store.srv.url}/healthz").status_code == 200
        else:
            other.close()  # the next request goes over a new connection
    store.delete("stays")
    store.wait_for(lambda m: m["s3d_recycle_busy_total"] == 1)
    store.delete_pooled("drops")
    other.close()


def test_concurrent_put_delete_cycles_keep_their_own_bytes(store):
    threads, cycles, n = 4, 6, 128 * KIB
    errors = []

    def worker(t):
        try:
            s = requests.Session()
            for c in range(cycles):
                data = pattern(n, 50 + t * cycles + c)
                key = f"t{t}/obj"
                assert s.put(f"{store.base}/{key}", data=data).status_code == 200
                r = s.get(f"{store.base}/{key}")
                assert r.status_code == 200 and r.content == data, (t, c)
                assert s.delete(f"{store.base}/{key}").status_code == 204
            s.close()
        except Exception as e:  # noqa: BLE001 - reported by the main thread
            errors.append(repr(e)[:300])

    ts = [threading.Thread(target=worker, args=(t,)) for t in range(threads)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert errors == []
    total = threads * cycles
    m = store.wait_for(lambda m: m["s3d_recycle_pooled_total"] + m["s3d_trash_unlinked_total"]
                       == total)
    assert m["s3d_recycle_hits_total"] > 0
    assert m["s3d_recycle_hits_total"] + m["s3d_recycle_pool_files"] == m["s3d_recycle_pooled_total"]
    assert store.srv.proc.poll() is None, "server died (sanitizer report?)"


def test_pool_stays_under_its_cap_and_restart_empties_it(tmp_path):
    n, count = 100000, 8
    cap = 3 * n + n // 2
    s = Store(tmp_path / "s3", "--recycle-cap-bytes", str(cap))
    try:
        for i in range(count):
            s.put(f"o{i}", pattern(n, 70 + i))
        for i in range(count):
            s.delete(f"o{i}")
        m = s.wait_for(lambda m: m["s3d_recycle_pooled_total"] + m["s3d_trash_unlinked_total"]
                       == count)
        assert m["s3d_recycle_cap_bytes"] == cap
        assert m["s3d_recycle_pooled_total"] == 3 and m["s3d_recycle_pool_bytes"] == 3 * n
        assert sum(os.path.getsize(f) for f in s.recycle_files()) == 3 * n <= cap
        assert "<Key>" not in requests.get(s.base).text
        s.stop()
        s.start()
        assert s.recycle_files() == []
        assert s.metrics()["s3d_recycle_pool_files"] == 0
    finally:
        s.stop()


def test_cap_zero_switches_the_pool_off(tmp_path):
    s = Store(tmp_path / "s3", "--recycle-cap-bytes", "0")
    try:
        data = pattern(100000, 90)
        for i in range(3):
            s.put(f"o{i}", data)
            s.delete(f"o{i}")
        m = s.wait_for(lambda m: m["s3d_trash_unlinked_total"] == 3)
        assert m["s3d_recycle_pooled_total"] == 0 and s.recycle_files() == []
        assert s.put("again", data).status_code == 200
        assert s.get("again").content == data
        assert s.metrics()["s3d_recycle_hits_total"] == 0
    finally:
        s.stop()
