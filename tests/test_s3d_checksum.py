"""modelx-s3d verifies x-amz-checksum-crc32c on presigned PUT and UploadPart
bodies: a matching value is stored and echoed, a wrong one is refused with
BadDigest and leaves nothing behind, a malformed one is an InvalidRequest,
and a request without the header is stored as before."""
import base64
import os

import pytest
import requests

from modelx_amd.client.registry import RegistryClient
from modelx_amd.wire import digest as dg
from modelx_amd.wire import types

from test_crc32c import ref_crc32c, seeded
from util_servers import start_modelxd_s3, start_s3d

HEADER = "x-amz-checksum-crc32c"


@pytest.fixture(scope="module")
def stack(tmp_path_factory):
    root = tmp_path_factory.mktemp("s3-data")
    s3d = start_s3d(str(root))
    mdx = start_modelxd_s3(s3d.url, redirect=True)
    yield mdx, str(root)
    mdx.stop()
    s3d.stop()


def files_under(root):
    """{relative path: bytes} of every file the store holds."""
    out = {}
    for d, _, names in os.walk(root):
        for n in names:
            with open(os.path.join(d, n), "rb") as f:
                out[os.path.relpath(os.path.join(d, n), root)] = f.read()
    return out


def header_of(crc: int) -> str:
    return base64.b64encode(crc.to_bytes(4, "big")).decode()


@pytest.mark.parametrize("multipart", [False, True], ids=["put", "upload-part"])
@pytest.mark.parametrize("case", ["right", "wrong", "malformed", "absent"])
def test_checksum_header(stack, case, multipart):
    mdx, root = stack
    data = seeded(70001, seed=f"{case}-{multipart}")
    desc = types.Descriptor(name="w.bin", media_type=types.MEDIA_TYPE_MODEL_FILE,
                            digest=dg.sha256_digest(data), size=len(data))
    extra = {"multipart": "true", "part-count": "2"} if multipart else None
    client = RegistryClient(mdx.url)
    loc = client.get_blob_location(f"ck/{case}", desc, "upload", extra=extra)
    client.session.close()  # an open keep-alive connection delays the server's exit
    part = loc.properties["parts"][0]
    body = data[:len(data) // 2] if multipart else data
    crc = ref_crc32c(body)
    value = {"right": header_of(crc), "wrong": header_of(crc ^ 1), "malformed": "AAAA",
             "absent": None}[case]
    headers = {HEADER: value} if value is not None else {}
    r = requests.request(part.get("method") or "PUT", part["url"], headers=headers, data=body)
    held = files_under(root)
    assert not [name for name in held if ".tmp" in name]
    if case in ("right", "absent"):
        assert r.status_code == 200
        assert r.headers.get(HEADER) == value
        assert body in held.values()
    else:
        assert r.status_code == 400
        assert ("BadDigest" if case == "wrong" else "InvalidRequest") in r.text
        assert body not in held.values()
