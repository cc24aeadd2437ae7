// modelx-s3d — bundled S3-compatible object server (MinIO stand-in).
//
// This environment has no network and no MinIO binary, so integration tests
// and benchmarks that exercise the presigned-redirect data plane (the
// reference's docker-compose pairs modelxd with MinIO) run against this
// server instead. It implements the S3 surface modelxd + the client engine
// use: presigned GET (with Range) / PUT, header-auth SigV4 control calls,
// ListObjectsV2, and the multipart-upload lifecycle. SigV4 signatures are
// verified for real — both auth paths prove the signer in sigv4.cpp against
// an independent verifier.
#include <dirent.h>
#include <fcntl.h>
#include <signal.h>
#include <sys/ioctl.h>
#include <sys/mman.h>
#include <sys/sendfile.h>
#include <sys/stat.h>
#include <sys/statvfs.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <thread>
#include <ctime>
#include <string>

#include "modelx/crc32c_core.hpp"
#include "modelx/http.hpp"
#include "modelx/sha256.hpp"
#include "modelx/sigv4.hpp"
#include "modelx/store.hpp"

using namespace modelx;

namespace {

struct S3dConfig {
  std::string root = "data/s3";
  std::string access_key = "modelx";
  std::string secret_key = "modelx123";
  std::string region = "us-east-1";
  bool verify_auth = true;
};

S3dConfig g_cfg;

std::string iso_time(time_t t) {
  struct tm tmv;
  gmtime_r(&t, &tmv);
  char buf[40];
  strftime(buf, sizeof buf, "%Y-%m-%dT%H:%M:%S.000Z", &tmv);
  return buf;
}

bool mkdirs_for(const std::string& filepath) {
  size_t pos = 0;
  while ((pos = filepath.find('/', pos + 1)) != std::string::npos) {
    std::string dir = filepath.substr(0, pos);
    if (mkdir(dir.c_str(), 0755) != 0 && errno != EEXIST) return false;
  }
  return true;
}

std::string xml_escape(const std::string& s) {
  std::string out;
  for (char c : s) {
    switch (c) {
      case '<': out += "&lt;"; break;
      case '>': out += "&gt;"; break;
      case '&': out += "&amp;"; break;
      default: out += c;
    }
  }
  return out;
}

// object path on disk: <root>/<bucket>/<key>
std::string obj_path(const std::string& bucket, const std::string& key) {
  return g_cfg.root + "/" + bucket + "/" + key;
}

std::string mpu_dir(const std::string& upload_id) { return g_cfg.root + "/.mpu/" + upload_id; }

// x-amz-checksum-crc32c: standard base64 of the checksum's four bytes, most
// significant first. False unless `v` is exactly that.
bool parse_crc32c_header(const std::string& v, uint32_t* out) {
  static const char kAlphabet[] =
      "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
  if (v.size() != 8 || v[6] != '=' || v[7] != '=') return false;
  uint64_t bits = 0;
  for (int i = 0; i < 6; i++) {
    const char* at = v[i] ? strchr(kAlphabet, v[i]) : nullptr;
    if (!at) return false;
    bits = (bits << 6) | static_cast<uint64_t>(at - kAlphabet);
  }
  if (bits & 0xF) return false;  // 36 bits carry 32: the pad bits are zero
  *out = static_cast<uint32_t>(bits >> 4);
  return true;
}

std::string format_crc32c_header(uint32_t crc) {
  static const char kAlphabet[] =
      "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
  uint64_t bits = static_cast<uint64_t>(crc) << 4;
  std::string v(8, '=');
  for (int i = 0; i < 6; i++) v[i] = kAlphabet[(bits >> (30 - 6 * i)) & 63];
  return v;
}

// ---- counters (GET /.metrics) ------------------------------------------------
// Where a PUT lane's time goes: blocked on the client (socket side) or in the
// store (file side: the copy plus tmpfs page setup), and what the trash
// collector spends freeing pages. Sums over the process's life.
struct Counters {
  std::atomic<uint64_t> put_count{0}, put_bytes{0};
  std::atomic<uint64_t> put_sock_ns{0}, put_file_ns{0};
  std::atomic<uint64_t> trash_unlink_ns{0}, trash_unlinked{0};
  // recycled files: PUTs served from the pool / not, files pooled, files
  // refused because a GET had them open, times the pool was emptied for space
  std::atomic<uint64_t> recycle_hits{0}, recycle_misses{0}, recycle_pooled{0};
  std::atomic<uint64_t> recycle_busy{0}, recycle_drains{0};
};
Counters g_ctr;

uint64_t now_ns() {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return static_cast<uint64_t>(ts.tv_sec) * 1000000000ull + static_cast<uint64_t>(ts.tv_nsec);
}

// One PUT's share of the counters, added on whichever path the PUT leaves by.
struct PutTimer {
  uint64_t sock_ns = 0, file_ns = 0;
  const int64_t* bytes;
  explicit PutTimer(const int64_t* b) : bytes(b) {}
  ~PutTimer() {
    g_ctr.put_count++;
    g_ctr.put_bytes += static_cast<uint64_t>(*bytes);
    g_ctr.put_sock_ns += sock_ns;
    g_ctr.put_file_ns += file_ns;
  }
};

// ---- recycled files ----------------------------------------------------------
// Deleted data files wait in <root>/.recycle/ for a PUT of their size class,
// which overwrites their pages in place instead of allocating fresh ones: on
// tmpfs that is the difference between a copy and a copy plus a page
// allocation, memcg charge, xarray insert and LRU add per 4 KiB, with the
// matching frees in the trash collector.
//
// The one hazard is a GET still reading a file that a PUT then overwrites.
// Every data-file open of a GET goes through open_for_read, which counts the
// reader on the file's inode under g_pool.mu; pool_offer checks that count
// under the same lock and refuses a file that has readers (it is unlinked as
// before, and its readers keep the old bytes). A file reaches pool_offer only
// after defer_delete renamed it out of its object path, so an open that comes
// after the check cannot reach that inode any more: opens are by object path.
//
// A reader does not end when sendfile returns: sendfile is zero-copy, and the
// bytes the peer has not read yet sit in the socket buffers as references to
// the file's pages, which a PUT into the recycled file would rewrite under
// them. So the count stays until the peer has shown that it read the
// response: its next request arrives on the same connection and was not
// already on its way while the response was being sent (a pipelining client
// proves nothing, its counts stay for good). A connection that ends, by
// either side, proves nothing either: what it read last stays counted, and
// such a file is unlinked when deleted, never pooled. t_conn holds one
// connection's counts; the server runs one thread per connection.
using FileId = std::pair<dev_t, ino_t>;

struct Pool {
  std::mutex mu;
  std::multimap<int64_t, std::string> by_size;  // size -> path under .recycle/
  int64_t bytes = 0;
  std::map<FileId, int> readers;
  uint64_t seq = 0;
  // set once in main(), before the first thread starts
  int64_t cap = 0;                // --recycle-cap-bytes; 0 = no pool
  // --recycle-min-bytes. Below about a MiB (256 pages) a file's page setup
  // costs less than the pool's rename and the index entry are worth.
  int64_t min_bytes = 1 << 20;
  // A multipart manifest is read by path without a reader count and is
  // always below 8 KiB; nothing that small is ever pooled.
  static constexpr int64_t kMinFloor = 8192;
};
Pool g_pool;

std::string recycle_dir() { return g_cfg.root + "/.recycle"; }

// A pooled file serves a PUT of `want` bytes when its size is in
// [want, want + want/4]: the PUT truncates it to `want` at the end, and
// freeing more than a quarter of it there would cost what recycling saves.
// The file has left the index when this returns, so no second PUT gets it.
std::string pool_take(int64_t want) {
  if (want < g_pool.min_bytes) return "";
  std::lock_guard<std::mutex> lk(g_pool.mu);
  auto it = g_pool.by_size.lower_bound(want);
  if (it == g_pool.by_size.end() || it->first > want + want / 4) {
    g_ctr.recycle_misses++;
    return "";
  }
  std::string file = it->second;
  g_pool.bytes -= it->first;
  g_pool.by_size.erase(it);
  g_ctr.recycle_hits++;
  return file;
}

// Moves a deleted file into the pool; false leaves it to the caller to unlink.
bool pool_offer(const std::string& file, const struct stat& st) {
  if (!S_ISREG(st.st_mode) || st.st_nlink != 1 || st.st_size < g_pool.min_bytes) return false;
  std::lock_guard<std::mutex> lk(g_pool.mu);
  if (g_pool.bytes + st.st_size > g_pool.cap) return false;
  if (g_pool.readers.count(FileId(st.st_dev, st.st_ino))) {
    g_ctr.recycle_busy++;
    return false;
  }
  std::string dst = recycle_dir() + "/" + std::to_string(g_pool.seq++);
  if (::rename(file.c_str(), dst.c_str()) != 0) return false;
  g_pool.by_size.emplace(st.st_size, dst);
  g_pool.bytes += st.st_size;
  g_ctr.recycle_pooled++;
  return true;
}

// Frees every pooled file (a PUT met ENOSPC).
void pool_drain() {
  std::multimap<int64_t, std::string> files;
  {
    std::lock_guard<std::mutex> lk(g_pool.mu);
    files.swap(g_pool.by_size);
    g_pool.bytes = 0;
  }
  for (auto& f : files) ::unlink(f.second.c_str());
  g_ctr.recycle_drains++;
}

// True once per PUT when a write failed for lack of space and the pool has
// been emptied to make some: the caller repeats the write.
bool made_space(bool* retried) {
  if (errno != ENOSPC || *retried) return false;
  *retried = true;
  pool_drain();
  return true;
}

// The temporary file of a PUT of `want` bytes (<= 0: length unknown): a
// recycled file renamed to `tmp` and opened as it is, or a fresh empty one.
// A recycled file is at least `want` long; the caller writes from offset 0
// and cuts it to length before renaming it into place.
int open_put_tmp(const std::string& tmp, int64_t want, bool* recycled) {
  *recycled = false;
  std::string pooled = want > 0 ? pool_take(want) : "";
  if (!pooled.empty()) {
    if (::rename(pooled.c_str(), tmp.c_str()) == 0) {
      int fd = ::open(tmp.c_str(), O_RDWR | O_CLOEXEC);
      if (fd >= 0) {
        *recycled = true;
        return fd;
      }
      ::unlink(tmp.c_str());
    } else {
      ::unlink(pooled.c_str());
    }
  }
  return ::open(tmp.c_str(), O_RDWR | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
}

// The reader counts of this thread's connection that may still be dropped.
struct ConnReads {
  std::vector<FileId> held;
  bool pipelined = false;  // seen once, the connection's counts all stay
};
thread_local ConnReads t_conn;

// Opens a data file for a GET and counts the reader on its inode, under
// g_pool.mu (see above). The caller closes the descriptor; the count stays
// with the connection until reads_consumed().
int open_for_read(const std::string& path) {
  std::lock_guard<std::mutex> lk(g_pool.mu);
  int fd = ::open(path.c_str(), O_RDONLY | O_CLOEXEC);
  if (fd < 0) return -1;
  struct stat st;
  if (::fstat(fd, &st) != 0) {
    ::close(fd);
    return -1;
  }
  FileId id(st.st_dev, st.st_ino);
  g_pool.readers[id]++;
  t_conn.held.push_back(id);
  return fd;
}

// After a GET's last byte went to the socket: request bytes that are already
// here were sent without waiting for this response, so this client's later
// requests say nothing about what it has read.
void reads_sent(http::Request& req) {
  if (t_conn.held.empty() || t_conn.pipelined) return;
  int sock = req.raw_fd_if_plain();  // -1: TLS, or bytes wait in the buffer
  int pending = 0;
  if (sock < 0 || ::ioctl(sock, FIONREAD, &pending) != 0 || pending > 0) t_conn.pipelined = true;
}

// A new request arrived on this connection: the peer has read the responses
// before it, and the files they came from may be pooled again.
void reads_consumed() {
  if (t_conn.held.empty()) return;
  if (!t_conn.pipelined) {
    std::lock_guard<std::mutex> lk(g_pool.mu);
    for (auto& id : t_conn.held) {
      auto it = g_pool.readers.find(id);
      if (it != g_pool.readers.end() && --it->second == 0) g_pool.readers.erase(it);
    }
  }
  t_conn.held.clear();
}

std::string render_metrics() {
  auto secs = [](const std::atomic<uint64_t>& ns) { return std::to_string(ns.load() * 1e-9); };
  std::string m;
  {
    std::lock_guard<std::mutex> lk(g_pool.mu);
    m += "s3d_recycle_pool_bytes " + std::to_string(g_pool.bytes) + "\n";
    m += "s3d_recycle_pool_files " + std::to_string(g_pool.by_size.size()) + "\n";
  }
  m += "s3d_recycle_cap_bytes " + std::to_string(g_pool.cap) + "\n";
  m += "s3d_recycle_min_bytes " + std::to_string(g_pool.min_bytes) + "\n";
  m += "s3d_recycle_hits_total " + std::to_string(g_ctr.recycle_hits.load()) + "\n";
  m += "s3d_recycle_misses_total " + std::to_string(g_ctr.recycle_misses.load()) + "\n";
  m += "s3d_recycle_pooled_total " + std::to_string(g_ctr.recycle_pooled.load()) + "\n";
  m += "s3d_recycle_busy_total " + std::to_string(g_ctr.recycle_busy.load()) + "\n";
  m += "s3d_recycle_drains_total " + std::to_string(g_ctr.recycle_drains.load()) + "\n";
  m += "s3d_put_total " + std::to_string(g_ctr.put_count.load()) + "\n";
  m += "s3d_put_bytes_total " + std::to_string(g_ctr.put_bytes.load()) + "\n";
  m += "s3d_put_socket_seconds_total " + secs(g_ctr.put_sock_ns) + "\n";
  m += "s3d_put_file_seconds_total " + secs(g_ctr.put_file_ns) + "\n";
  m += "s3d_trash_unlink_seconds_total " + secs(g_ctr.trash_unlink_ns) + "\n";
  m += "s3d_trash_unlinked_total " + std::to_string(g_ctr.trash_unlinked.load()) + "\n";
  return m;
}

// Stores the request body at `path` through a temporary file. With
// `expect_crc32c` the body goes through user space (no splice), is
// checksummed as it is written, and is renamed into place only if its
// CRC-32C is *expect_crc32c; a mismatch removes the temporary file, sets
// *bad_digest and returns false. The temporary file is a recycled one when
// the pool has one of the body's size class (open_put_tmp); a write that
// fails with ENOSPC empties the pool and is repeated once.
bool write_stream_to(const std::string& path, http::Request& req, std::string* etag,
                     const uint32_t* expect_crc32c = nullptr, bool* bad_digest = nullptr) {
  if (!mkdirs_for(path)) return false;
  std::string tmp = path + ".tmp" + std::to_string(getpid());
  bool recycled = false;
  int fd = open_put_tmp(tmp, req.content_length, &recycled);
  if (fd < 0) return false;
  int64_t total = 0;
  PutTimer timer(&total);
  bool retried = false;  // made_space: one retry per PUT
  // Closes the temporary file, cut to the body's length where it came from
  // the pool (a recycled file may be longer and then holds a stale tail).
  auto close_at_length = [&]() {
    bool ok = !recycled || ::ftruncate(fd, total) == 0;
    ::close(fd);
    return ok;
  };
  // NOTE: an mmap+recv variant (ftruncate, MAP_SHARED, recv into the
  // mapping) was A/B-tested on the GPU box and LOST to plain write() on the
  // tmpfs store: per-page fault handling in the recv copy path costs more
  // than the buffer bounce it saves (push throughput 7.5 vs 12.5 GiB/s).
  // splice(socket->pipe->file) sink: zero user-space copies; measured
  // faster than the write() loop on the GPU box (bench push+pull 15.3 vs
  // 14.3 GiB/s at equal settings). MODELX_S3D_SPLICE=0 opts out.
  static const bool use_splice = [] {
    const char* v = getenv("MODELX_S3D_SPLICE");
    return !(v && *v == '0');
  }();
  if (use_splice && req.content_length > 0 && !expect_crc32c) {
    // drain any bytes the header parser buffered first
    char small[16384];
    while (req.body_remaining > 0 && req.raw_fd_if_plain() < 0) {
      ssize_t r = req.read_body(small, sizeof small);
      if (r <= 0) break;
      ssize_t off = 0;
      while (off < r) {
        ssize_t w = ::write(fd, small + off, static_cast<size_t>(r - off));
        if (w < 0 && (errno == EINTR || made_space(&retried))) continue;
        if (w < 0) {
          // counting unwritten bytes would let a short object pass the
          // completeness check below and be renamed into place
          ::close(fd);
          ::unlink(tmp.c_str());
          return false;
        }
        off += w;
      }
      total += r;
    }
    int sock = req.raw_fd_if_plain();
    if (sock >= 0 && req.body_remaining > 0) {
      int pfd[2];
      if (::pipe(pfd) == 0) {
        fcntl(pfd[0], F_SETPIPE_SZ, 1 << 20);
        int64_t rem = req.body_remaining;
        while (rem > 0) {
          uint64_t t0 = now_ns();
          ssize_t r = ::splice(sock, nullptr, pfd[1], nullptr,
                               static_cast<size_t>(std::min<int64_t>(rem, 1 << 20)),
                               SPLICE_F_MOVE | SPLICE_F_MORE);
          uint64_t t1 = now_ns();
          timer.sock_ns += t1 - t0;
          if (r < 0 && errno == EINTR) continue;
          if (r <= 0) break;
          ssize_t moved = 0;
          while (moved < r) {
            ssize_t w = ::splice(pfd[0], nullptr, fd, nullptr,
                                 static_cast<size_t>(r - moved), SPLICE_F_MOVE);
            // the bytes are still in the pipe after a failed splice
            if (w < 0 && (errno == EINTR || made_space(&retried))) continue;
            if (w <= 0) { moved = -1; break; }
            moved += w;
          }
          timer.file_ns += now_ns() - t1;
          if (moved < 0) break;
          rem -= r;
          total += r;
        }
        req.body_remaining = rem;
        ::close(pfd[0]);
        ::close(pfd[1]);
      }
    }
    if (!close_at_length() || total != req.content_length) {
      ::unlink(tmp.c_str());
      return false;
    }
    if (::rename(tmp.c_str(), path.c_str()) != 0) {
      ::unlink(tmp.c_str());
      return false;
    }
    if (etag) *etag = "\"s3d-" + std::to_string(total) + "\"";
    return true;
  }
  std::vector<char> buf(4 << 20);
  uint32_t crc = crc32c::kInit;
  while (true) {
    uint64_t t0 = now_ns();
    ssize_t r = req.read_body(buf.data(), buf.size());
    uint64_t t1 = now_ns();
    timer.sock_ns += t1 - t0;
    if (r < 0) {
      ::close(fd);
      ::unlink(tmp.c_str());
      return false;
    }
    if (r == 0) break;
    if (expect_crc32c) crc = crc32c::update(crc, buf.data(), static_cast<size_t>(r));
    ssize_t off = 0;
    while (off < r) {
      ssize_t w = ::write(fd, buf.data() + off, static_cast<size_t>(r - off));
      if (w < 0) {
        if (errno == EINTR || made_space(&retried)) continue;
        ::close(fd);
        ::unlink(tmp.c_str());
        return false;
      }
      off += w;
    }
    timer.file_ns += now_ns() - t1;
    total += r;
  }
  if (!close_at_length() || total != req.content_length) {
    ::unlink(tmp.c_str());
    return false;
  }
  if (expect_crc32c && (crc ^ crc32c::kInit) != *expect_crc32c) {
    ::unlink(tmp.c_str());
    if (bad_digest) *bad_digest = true;
    return false;
  }
  if (::rename(tmp.c_str(), path.c_str()) != 0) {
    ::unlink(tmp.c_str());
    return false;
  }
  if (etag) *etag = "\"s3d-" + std::to_string(total) + "\"";
  return true;
}

// The body of a PUT object or UploadPart into `path`, verified against the
// request's x-amz-checksum-crc32c when it carries one. Returns true when the
// bytes are in place; otherwise the error response has been written. A
// request without the header takes write_stream_to's usual path, splice
// included.
bool store_put_body(const std::string& path, http::Request& req, http::ResponseWriter& w,
                    std::string* etag) {
  auto ck = req.headers.find("x-amz-checksum-crc32c");
  uint32_t want = 0;
  bool checked = ck != req.headers.end();
  if (checked && !parse_crc32c_header(ck->second, &want)) {
    // before any body byte is stored; the server loop drains the unread body
    w.write_all(400,
                "<Error><Code>InvalidRequest</Code><Message>Value for x-amz-checksum-crc32c "
                "header is invalid.</Message></Error>",
                "application/xml");
    return false;
  }
  bool bad_digest = false;
  if (!write_stream_to(path, req, etag, checked ? &want : nullptr, &bad_digest)) {
    if (bad_digest)
      w.write_all(400,
                  "<Error><Code>BadDigest</Code><Message>The CRC32C you specified did not "
                  "match the calculated checksum.</Message></Error>",
                  "application/xml");
    else
      w.write_all(500, "<Error><Code>InternalError</Code></Error>", "application/xml");
    return false;
  }
  if (checked) w.set_header("x-amz-checksum-crc32c", format_crc32c_header(want));
  return true;
}

bool authorized(http::Request& req) {
  if (!g_cfg.verify_auth) return true;
  sigv4::Credentials cred{g_cfg.access_key, g_cfg.secret_key, g_cfg.region, "s3"};
  std::string host;
  auto hit = req.headers.find("Host");
  if (hit != req.headers.end()) host = hit->second;
  if (req.query.count("X-Amz-Signature")) {
    std::string err;
    // NOTE: raw (encoded) path must be re-derived: our Request.path is decoded,
    // but modelx keys contain no chars needing encoding beyond what
    // url_encode_path leaves alone, so re-encoding is canonical.
    std::string raw_path = http::url_encode_path(req.path);
    return sigv4::verify_presigned(req.method, raw_path, req.query, host, cred, time(nullptr),
                                   &err);
  }
  auto ait = req.headers.find("Authorization");
  if (ait == req.headers.end()) return false;
  const std::string& auth = ait->second;
  // AWS4-HMAC-SHA256 Credential=AK/scope, SignedHeaders=a;b, Signature=hex
  size_t sh = auth.find("SignedHeaders=");
  size_t sig = auth.find("Signature=");
  size_t crd = auth.find("Credential=");
  if (sh == std::string::npos || sig == std::string::npos || crd == std::string::npos)
    return false;
  std::string cred_str = auth.substr(crd + 11, auth.find(',', crd) - crd - 11);
  if (cred_str.substr(0, cred_str.find('/')) != g_cfg.access_key) return false;
  std::string signed_headers = auth.substr(sh + 14, auth.find(',', sh) - sh - 14);
  std::string given_sig = auth.substr(sig + 10);
  // recompute
  sigv4::RequestToSign rts;
  rts.method = req.method;
  rts.path = http::url_encode_path(req.path);
  for (auto& kv : req.query)
    rts.query[http::url_encode_query(kv.first)] = http::url_encode_query(kv.second);
  auto xs = req.headers.find("x-amz-content-sha256");
  rts.payload_hash = xs != req.headers.end() ? xs->second : "UNSIGNED-PAYLOAD";
  std::string amz_date;
  auto xd = req.headers.find("x-amz-date");
  if (xd != req.headers.end()) amz_date = xd->second;
  // build headers map exactly from SignedHeaders list
  std::map<std::string, std::string> hmap;
  size_t pos = 0;
  while (pos <= signed_headers.size()) {
    size_t semi = signed_headers.find(';', pos);
    if (semi == std::string::npos) semi = signed_headers.size();
    std::string h = signed_headers.substr(pos, semi - pos);
    pos = semi + 1;
    if (h.empty()) continue;
    if (h == "host") {
      hmap["host"] = host;
    } else {
      auto it = req.headers.find(h);
      hmap[h] = it != req.headers.end() ? it->second : "";
    }
  }
  rts.headers = hmap;
  // sign_authorization rebuilds canonical from rts.headers
  std::string expect = sigv4::sign_authorization(rts, cred, amz_date);
  size_t esig = expect.find("Signature=");
  return esig != std::string::npos && expect.substr(esig + 10) == given_sig;
}

// ---- deferred deletion -----------------------------------------------------
std::mutex g_trash_mu;
std::condition_variable g_trash_cv;
std::deque<std::string> g_trash_queue;
std::atomic<uint64_t> g_trash_seq{0};

void defer_delete(const std::string& path) {
  std::string trash_dir = g_cfg.root + "/.trash";
  mkdirs_for(trash_dir + "/x");
  uint64_t seq = g_trash_seq.fetch_add(1);
  ::unlink((path + ".ct").c_str());
  bool queued = false;
  std::string t1 = trash_dir + "/" + std::to_string(getpid()) + "-" + std::to_string(seq);
  if (::rename(path.c_str(), t1.c_str()) == 0) {
    queued = true;
  }
  std::string t2 = t1 + ".parts";
  if (::rename((path + ".parts").c_str(), t2.c_str()) == 0) queued = true;
  if (queued) {
    {
      std::lock_guard<std::mutex> lk(g_trash_mu);
      g_trash_queue.push_back(t1);
      g_trash_queue.push_back(t2);
    }
    g_trash_cv.notify_one();
  }
}

// Disposes of one trashed path: a directory (an object's parts) file by
// file, a file into the recycle pool where it qualifies, else unlinked.
void collect(const std::string& victim) {
  struct stat st;
  if (::lstat(victim.c_str(), &st) != 0) return;
  if (S_ISDIR(st.st_mode)) {
    std::vector<std::string> names;
    if (DIR* d = ::opendir(victim.c_str())) {
      while (struct dirent* e = ::readdir(d)) {
        std::string n = e->d_name;
        if (n != "." && n != "..") names.push_back(n);
      }
      ::closedir(d);
    }
    for (auto& n : names) collect(victim + "/" + n);
    ::rmdir(victim.c_str());
    return;
  }
  if (pool_offer(victim, st)) return;
  uint64_t t0 = now_ns();
  ::unlink(victim.c_str());
  g_ctr.trash_unlink_ns += now_ns() - t0;
  g_ctr.trash_unlinked++;
}

void trash_collector() {
  while (true) {
    std::string victim;
    {
      std::unique_lock<std::mutex> lk(g_trash_mu);
      g_trash_cv.wait(lk, [] { return !g_trash_queue.empty(); });
      victim = g_trash_queue.front();
      g_trash_queue.pop_front();
    }
    collect(victim);
  }
}

void list_objects(http::Request& req, http::ResponseWriter& w, const std::string& bucket) {
  std::string prefix = req.query.count("prefix") ? req.query["prefix"] : "";
  bool delimited = req.query.count("delimiter") > 0;
  store::LocalFSProvider fs(g_cfg.root + "/" + bucket);
  // reuse LocalFSProvider's recursive walk; prefix may be a partial path
  std::string dir_part = prefix;
  std::string name_part;
  size_t slash = prefix.rfind('/');
  if (slash != std::string::npos) {
    dir_part = prefix.substr(0, slash);
    name_part = prefix.substr(slash + 1);
  } else {
    dir_part = "";
    name_part = prefix;
  }
  auto metas = fs.List(dir_part, !delimited);
  std::string xml = "<?xml version=\"1.0\"?><ListBucketResult>";
  xml += "<IsTruncated>false</IsTruncated>";
  int count = 0;
  for (auto& m : metas) {
    std::string key = dir_part.empty() ? m.name : dir_part + "/" + m.name;
    if (!prefix.empty() && key.compare(0, prefix.size(), prefix) != 0) continue;
    if (key.find(".parts/") != std::string::npos) continue;  // internal multipart storage
    if (key.size() > 3 && key.compare(key.size() - 3, 3, ".ct") == 0) continue;
    xml += "<Contents><Key>" + xml_escape(key) + "</Key><Size>" + std::to_string(m.size) +
           "</Size><LastModified>" + m.last_modified + "</LastModified></Contents>";
    if (++count >= 100000) break;
  }
  xml += "</ListBucketResult>";
  w.write_all(200, xml, "application/xml");
}

void list_uploads(http::Request& req, http::ResponseWriter& w, const std::string& bucket) {
  std::string prefix = req.query.count("prefix") ? req.query["prefix"] : "";
  std::string xml = "<?xml version=\"1.0\"?><ListMultipartUploadsResult>";
  store::LocalFSProvider fs(g_cfg.root + "/.mpu");
  for (auto& m : fs.List("", true)) {
    // entries are "<uploadId>/.keyinfo"
    size_t slash = m.name.find('/');
    if (slash == std::string::npos || m.name.substr(slash + 1) != ".keyinfo") continue;
    std::string upload_id = m.name.substr(0, slash);
    std::string info;
    if (!fs.GetBytes(m.name, &info)) continue;
    // info = "<bucket>\n<key>"
    size_t nl = info.find('\n');
    if (nl == std::string::npos) continue;
    std::string ub = info.substr(0, nl), uk = info.substr(nl + 1);
    if (ub != bucket) continue;
    if (!prefix.empty() && uk.compare(0, prefix.size(), prefix) != 0) continue;
    xml += "<Upload><Key>" + xml_escape(uk) + "</Key><UploadId>" + upload_id +
           "</UploadId></Upload>";
  }
  xml += "</ListMultipartUploadsResult>";
  w.write_all(200, xml, "application/xml");
}

void list_parts(http::Request& req, http::ResponseWriter& w, const std::string& upload_id) {
  std::string xml = "<?xml version=\"1.0\"?><ListPartsResult>";
  store::LocalFSProvider fs(mpu_dir(upload_id));
  auto metas = fs.List("", false);
  std::vector<std::pair<int, int64_t>> parts;
  for (auto& m : metas) {
    if (m.name == ".keyinfo") continue;
    parts.emplace_back(atoi(m.name.c_str()), m.size);
  }
  std::sort(parts.begin(), parts.end());
  for (auto& p : parts) {
    xml += "<Part><PartNumber>" + std::to_string(p.first) + "</PartNumber><ETag>\"s3d-" +
           std::to_string(p.second) + "\"</ETag><Size>" + std::to_string(p.second) +
           "</Size></Part>";
  }
  xml += "</ListPartsResult>";
  w.write_all(200, xml, "application/xml");
}

// Multipart completion is ZERO-COPY: parts are renamed under
// "<object>.parts/<n>" and a tiny "<object>" manifest file records the
// layout ("S3DPARTS\n<size part>\n..."). GET/HEAD serve ranges across part
// files with sendfile. (A byte-concat completion — what a naive stand-in
// does — costs a full extra write of the object and was ~30% of a bench
// step; real S3 also keeps parts separate internally.)
constexpr const char* kPartsMagic = "S3DPARTS\n";

struct PartsManifest {
  std::vector<std::pair<int64_t, std::string>> parts;  // size, path
  int64_t total = 0;
};

bool load_parts_manifest(const std::string& path, PartsManifest* out) {
  int fd = ::open(path.c_str(), O_RDONLY | O_CLOEXEC);
  if (fd < 0) return false;
  char buf[8192];
  ssize_t r = ::read(fd, buf, sizeof buf - 1);
  ::close(fd);
  if (r < static_cast<ssize_t>(strlen(kPartsMagic))) return false;
  buf[r] = 0;
  if (strncmp(buf, kPartsMagic, strlen(kPartsMagic)) != 0) return false;
  const char* p = buf + strlen(kPartsMagic);
  while (*p) {
    char name[64];
    long long sz;
    int n = 0;
    if (sscanf(p, "%lld %63s%n", &sz, name, &n) != 2) break;
    out->parts.emplace_back(sz, path + ".parts/" + name);
    out->total += sz;
    p += n;
    while (*p == '\n' || *p == ' ') p++;
  }
  return !out->parts.empty();
}

void complete_multipart(http::Request& req, http::ResponseWriter& w, const std::string& bucket,
                        const std::string& key, const std::string& upload_id) {
  req.read_body_all(16 << 20);  // part list XML (we trust our ListParts order)
  std::string dir = mpu_dir(upload_id);
  store::LocalFSProvider fs(dir);
  std::vector<std::pair<int, std::string>> parts;
  for (auto& m : fs.List("", false)) {
    if (m.name == ".keyinfo") continue;
    parts.emplace_back(atoi(m.name.c_str()), m.name);
  }
  if (parts.empty()) {
    w.write_all(400, "<Error><Code>InvalidPart</Code></Error>", "application/xml");
    return;
  }
  std::sort(parts.begin(), parts.end());
  std::string dest = obj_path(bucket, key);
  mkdirs_for(dest);
  if (parts.size() == 1) {
    if (::rename((dir + "/" + parts[0].second).c_str(), dest.c_str()) != 0) {
      w.write_all(500, "<Error><Code>InternalError</Code></Error>", "application/xml");
      return;
    }
  } else {
    std::string pdir = dest + ".parts";
    store::LocalFSProvider(g_cfg.root).Remove(
        pdir.substr(g_cfg.root.size() + 1), true);  // stale parts from a prior object
    mkdirs_for(pdir + "/x");
    std::string manifest = kPartsMagic;
    bool ok = true;
    for (auto& p : parts) {
      struct stat st;
      std::string src = dir + "/" + p.second;
      if (::stat(src.c_str(), &st) != 0 ||
          ::rename(src.c_str(), (pdir + "/" + p.second).c_str()) != 0) {
        ok = false;
        break;
      }
      manifest += std::to_string((long long)st.st_size) + " " + p.second + "\n";
    }
    std::string tmp = dest + ".tmp" + std::to_string(getpid());
    // a fresh file: a manifest is below the smallest file the pool keeps
    int out = ok ? ::open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644) : -1;
    if (out >= 0) {
      ok = ::write(out, manifest.data(), manifest.size()) ==
           static_cast<ssize_t>(manifest.size());
      ::close(out);
    } else {
      ok = false;
    }
    if (!ok || ::rename(tmp.c_str(), dest.c_str()) != 0) {
      ::unlink(tmp.c_str());
      w.write_all(500, "<Error><Code>InternalError</Code></Error>", "application/xml");
      return;
    }
  }
  // drop upload state
  store::LocalFSProvider root(g_cfg.root);
  root.Remove(".mpu/" + upload_id, true);
  std::string xml = "<?xml version=\"1.0\"?><CompleteMultipartUploadResult><Key>" +
                    xml_escape(key) + "</Key></CompleteMultipartUploadResult>";
  w.write_all(200, xml, "application/xml");
}

void handle(http::Request& req, http::ResponseWriter& w) {
  reads_consumed();
  if (req.path == "/healthz") {
    w.write_all(200, "ok");
    return;
  }
  // counters only, open like /healthz; a dot name can be no bucket's
  if (req.path == "/.metrics" && req.method == "GET") {
    w.write_all(200, render_metrics(), "text/plain; version=0.0.4");
    return;
  }
  if (!authorized(req)) {
    fprintf(stderr, "s3d: auth failed: %s %s\n", req.method.c_str(), req.target.c_str());
    w.write_all(403, "<Error><Code>SignatureDoesNotMatch</Code></Error>", "application/xml");
    return;
  }
  // /<bucket>[/<key...>]
  std::string p = req.path;
  if (p.empty() || p[0] != '/') {
    w.write_all(404, "bad path");
    return;
  }
  size_t slash = p.find('/', 1);
  std::string bucket = slash == std::string::npos ? p.substr(1) : p.substr(1, slash - 1);
  std::string key = slash == std::string::npos ? "" : p.substr(slash + 1);
  // .mpu, .trash and .recycle hold the server's own files, never objects
  if (bucket.empty() || bucket[0] == '.') {
    w.write_all(404, "no bucket");
    return;
  }

  if (key.empty()) {
    // bucket-level ops
    if (req.method == "GET" && req.query.count("uploads")) return list_uploads(req, w, bucket);
    if (req.method == "GET") return list_objects(req, w, bucket);
    if (req.method == "PUT") {  // create bucket
      mkdirs_for(g_cfg.root + "/" + bucket + "/.");
      w.write_all(200, "");
      return;
    }
    if (req.method == "HEAD") {
      struct stat st;
      bool ok = ::stat((g_cfg.root + "/" + bucket).c_str(), &st) == 0 && S_ISDIR(st.st_mode);
      w.write_all(ok ? 200 : 404, "");
      return;
    }
    w.write_all(405, "");
    return;
  }

  std::string path = obj_path(bucket, key);

  if (req.method == "POST" && req.query.count("uploads")) {
    // initiate multipart
    std::string upload_id = sha256_hex(bucket + "/" + key + std::to_string(time(nullptr)) +
                                       std::to_string(rand()))
                                .substr(0, 32);
    store::LocalFSProvider root(g_cfg.root);
    root.PutBytes(".mpu/" + upload_id + "/.keyinfo", "text/plain", bucket + "\n" + key);
    std::string xml = "<?xml version=\"1.0\"?><InitiateMultipartUploadResult><Bucket>" + bucket +
                      "</Bucket><Key>" + xml_escape(key) + "</Key><UploadId>" + upload_id +
                      "</UploadId></InitiateMultipartUploadResult>";
    w.write_all(200, xml, "application/xml");
    return;
  }
  if (req.method == "POST" && req.query.count("uploadId"))
    return complete_multipart(req, w, bucket, key, req.query["uploadId"]);
  if (req.method == "GET" && req.query.count("uploadId"))
    return list_parts(req, w, req.query["uploadId"]);
  if (req.method == "PUT" && req.query.count("partNumber") && req.query.count("uploadId")) {
    int part = atoi(req.query["partNumber"].c_str());
    char name[16];
    snprintf(name, sizeof name, "%06d", part);
    std::string ppath = mpu_dir(req.query["uploadId"]) + "/" + name;
    std::string etag;
    if (!store_put_body(ppath, req, w, &etag)) return;
    w.set_header("ETag", etag);
    w.write_all(200, "");
    return;
  }

  if (req.method == "PUT") {
    std::string etag;
    if (!store_put_body(path, req, w, &etag)) return;
    // content-type sidecar so HEAD/GET can return it
    auto ct = req.headers.find("Content-Type");
    if (ct != req.headers.end() && !ct->second.empty()) {
      int fd = ::open((path + ".ct").c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
      if (fd >= 0) {
        ssize_t unused = ::write(fd, ct->second.data(), ct->second.size());
        (void)unused;
        ::close(fd);
      }
    }
    w.set_header("ETag", etag);
    w.write_all(200, "");
    return;
  }

  if (req.method == "HEAD" || req.method == "GET") {
    struct stat st;
    if (::stat(path.c_str(), &st) != 0 || !S_ISREG(st.st_mode)) {
      w.write_all(404, "<Error><Code>NoSuchKey</Code></Error>", "application/xml");
      return;
    }
    PartsManifest pm;
    bool is_parts = st.st_size < 8192 && load_parts_manifest(path, &pm);
    int64_t object_size = is_parts ? pm.total : st.st_size;
    std::string ctype = "application/octet-stream";
    {
      int fd = ::open((path + ".ct").c_str(), O_RDONLY | O_CLOEXEC);
      if (fd >= 0) {
        char buf[256];
        ssize_t r = ::read(fd, buf, sizeof buf);
        ::close(fd);
        if (r > 0) ctype.assign(buf, static_cast<size_t>(r));
      }
    }
    st.st_size = object_size;
    int64_t start = 0, length = st.st_size;
    int status = 200;
    auto rit = req.headers.find("Range");
    if (rit != req.headers.end() && rit->second.rfind("bytes=", 0) == 0) {
      std::string spec = rit->second.substr(6);
      size_t dash = spec.find('-');
      if (dash != std::string::npos) {
        std::string a = spec.substr(0, dash), b = spec.substr(dash + 1);
        if (!a.empty()) {
          start = atoll(a.c_str());
          int64_t end = b.empty() ? st.st_size - 1 : atoll(b.c_str());
          if (start >= st.st_size) {
            w.write_all(416, "");
            return;
          }
          end = std::min<int64_t>(end, st.st_size - 1);
          length = end - start + 1;
          status = 206;
          w.set_header("Content-Range", "bytes " + std::to_string(start) + "-" +
                                            std::to_string(end) + "/" +
                                            std::to_string(st.st_size));
        } else if (!b.empty()) {  // suffix range
          int64_t n = atoll(b.c_str());
          start = std::max<int64_t>(0, st.st_size - n);
          length = st.st_size - start;
          status = 206;
          w.set_header("Content-Range", "bytes " + std::to_string(start) + "-" +
                                            std::to_string(st.st_size - 1) + "/" +
                                            std::to_string(st.st_size));
        }
      }
    }
    w.set_header("Content-Type", ctype);
    w.set_header("Last-Modified", iso_time(st.st_mtime));
    w.set_header("Accept-Ranges", "bytes");
    w.begin(status, length);
    if (req.method == "GET") {
      bool delivered = false;
      if (!is_parts) {
        int fd = open_for_read(path);
        if (fd >= 0) {
          delivered = w.sendfile(fd, start, length);
          ::close(fd);
        }
      } else {
        // stitch the range across part files (zero-copy sendfile per part)
        int64_t pos = 0, remaining = length, cursor = start;
        for (auto& part : pm.parts) {
          if (remaining <= 0) break;
          int64_t psize = part.first;
          if (cursor >= pos + psize) {
            pos += psize;
            continue;
          }
          int64_t in_off = cursor - pos;
          int64_t take = std::min(psize - in_off, remaining);
          int fd = open_for_read(part.second);
          if (fd < 0) break;
          bool ok = w.sendfile(fd, in_off, take);
          ::close(fd);
          if (!ok) break;
          cursor += take;
          remaining -= take;
          pos += psize;
        }
        delivered = remaining == 0;
      }
      // promised Content-Length but couldn't deliver: the stream is
      // desynced — close the connection so the client fails loudly and
      // retries, instead of reading the next response as body bytes
      if (!delivered) w.abort_connection();
      reads_sent(req);
    }
    return;
  }

  if (req.method == "DELETE") {
    // deferred deletion: rename into .trash (fast) and let the collector
    // thread unlink — freeing GiBs of tmpfs pages synchronously would stall
    // the request path for hundreds of ms
    defer_delete(path);
    w.write_all(204, "");
    return;
  }
  w.write_all(405, "");
}

}  // namespace

int main(int argc, char** argv) {
  std::string listen = ":9000";
  http::TlsConfig tls;
  int64_t recycle_cap = -1;  // -1: derive from the filesystem below
  for (int i = 1; i < argc; i++) {
    std::string a = argv[i];
    auto next = [&]() -> std::string { return i + 1 < argc ? argv[++i] : ""; };
    if (a == "--listen") listen = next();
    else if (a == "--root") g_cfg.root = next();
    else if (a == "--access-key") g_cfg.access_key = next();
    else if (a == "--secret-key") g_cfg.secret_key = next();
    else if (a == "--region") g_cfg.region = next();
    else if (a == "--no-auth") g_cfg.verify_auth = false;
    else if (a == "--tls-cert") tls.cert_file = next();
    else if (a == "--tls-key") tls.key_file = next();
    else if (a == "--recycle-cap-bytes") recycle_cap = atoll(next().c_str());
    else if (a == "--recycle-min-bytes")
      g_pool.min_bytes = std::max<int64_t>(Pool::kMinFloor, atoll(next().c_str()));
    else if (a == "--help" || a == "-h") {
      printf("modelx-s3d: S3-compatible test/bench object server\n"
             "  --listen :9000  --root data/s3  --access-key K --secret-key S\n"
             "  --region us-east-1  --no-auth  --tls-cert F --tls-key F\n"
             "  --recycle-cap-bytes N (default: 1/4 of the root's free space; 0 = off)\n"
             "  --recycle-min-bytes N (default 1 MiB, at least 8 KiB)\n");
      return 0;
    }
  }
  signal(SIGPIPE, SIG_IGN);
  mkdirs_for(g_cfg.root + "/.");
  // nothing under these two outlives the process that put it there
  store::LocalFSProvider(g_cfg.root).Remove(".trash", true);
  store::LocalFSProvider(g_cfg.root).Remove(".recycle", true);
  mkdirs_for(recycle_dir() + "/.");
  if (recycle_cap < 0) {
    struct statvfs vfs;
    recycle_cap = ::statvfs(g_cfg.root.c_str(), &vfs) == 0
                      ? static_cast<int64_t>(vfs.f_bavail) * static_cast<int64_t>(vfs.f_frsize) / 4
                      : 0;
  }
  g_pool.cap = recycle_cap;
  std::thread(trash_collector).detach();
  http::Server server(listen, handle, tls);
  int port = server.start();
  printf("modelx-s3d listening on port %d root=%s\n", port, g_cfg.root.c_str());
  fflush(stdout);
  // run until signaled
  sigset_t set;
  sigemptyset(&set);
  sigaddset(&set, SIGINT);
  sigaddset(&set, SIGTERM);
  sigprocmask(SIG_BLOCK, &set, nullptr);
  int sig = 0;
  sigwait(&set, &sig);
  server.stop();
  // The collector and the connection threads are detached and still use the
  // globals above; returning would run their destructors under them (a
  // condition variable with a waiter never finishes being destroyed).
  fflush(nullptr);
  _exit(0);
}
