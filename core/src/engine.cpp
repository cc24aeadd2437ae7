// Pinned-ring S3→HBM streaming engine (+ pybind11 bindings → modelx_amd._core).
//
// MI355X-native replacement for the reference's io.Copy download chain
// (reference: pkg/client/extension_http.go:11-29, extension_s3.go:24-37 —
// single-stream, CPU-file destination). Design:
//
//   socket (ranged GET, N conns) ──► pinned host slot ──► hipMemcpyAsync
//        (downloader threads)          (ring of slots)      (per-slot stream)
//                                                              │
//                              reclaimer thread ◄── hipEvent ──┘
//
//  - N keep-alive connections issue ranged GETs against ONE presigned URL
//    (Range is outside the SigV4 signature, SignedHeaders=host)
//  - each range lands in a pinned slot; recv() writes straight into pinned
//    memory, so the H2D DMA needs no extra copy
//  - H2D copies run on a small pool of side streams, overlapped with the
//    next range's socket reads; a reclaimer thread returns slots on event
//    completion, so the ring never blocks a downloader on DMA
//  - after landing, the CDNA4 SHA-256 chunk kernel (core/hip/sha256.hip)
//    verifies the chunked digest at HBM-class rate, off the transfer's
//    critical path
//
// The same ring runs push: device → pinned slot (D2H) → multipart PUT parts.
#include <hip/hip_runtime.h>
#include <openssl/evp.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <queue>
#include <stdexcept>
#include <string_view>
#include <thread>
#include <unordered_set>
#include <vector>

#include "modelx/byteplane_host.hpp"
#include "modelx/device_abi.hpp"
#include "modelx/http.hpp"
#include "modelx/tar_host.hpp"
#include "modelx/zstd_core.hpp"
#include "modelx/zstd_host.hpp"

namespace py = pybind11;
using namespace modelx;
using modelx::abi::ChunkLeavesDesc;
using modelx::abi::CopySeg;
using modelx::abi::kDedupMaxProbes;
using modelx::abi::PackSeg;
using modelx::abi::TarEntry;
using modelx::abi::TarWalkResult;
using zstdhost::SeekEntry;

// MODELX_ZSTD_FLAGS: bit0 disables the lane-parallel huffman encoder,
// bit1 disables the wave-split literal-stream decoder (bisection/panic
// switches for the device codec); bit2 (value 4) makes every compress
// literals-only (no LZ parse) — zstd_compress_device(literals_only=true) sets
// it for one launch, which is how byte-plane blobs are encoded.
static uint32_t zstd_flags() {
  static uint32_t f = [] {
    const char* v = getenv("MODELX_ZSTD_FLAGS");
    return v ? (uint32_t)atoi(v) : 0u;
  }();
  return f;
}

#define HIP_CHECK(expr)                                                                 \
  do {                                                                                  \
    hipError_t _e = (expr);                                                             \
    if (_e != hipSuccess)                                                               \
      throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(_e) +     \
                               " at " #expr);                                           \
  } while (0)

namespace {

double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

// Leaves a blob of `size` bytes has at `chunk_size` (> 0): an empty blob has
// the one leaf of the empty string.
uint64_t expected_leaf_count(uint64_t size, uint64_t chunk_size) {
  return size ? (size - 1) / chunk_size + 1 : 1;
}

// Leaf count of a packed 32 B/leaf array, or a throw when it is not the
// array of a `size`-byte blob at `chunk_size`. The dedup kernels derive
// every chunk address from (index, chunk_size, size): a surplus leaf would
// address memory past the blob.
uint32_t checked_leaf_count(const char* who, size_t leaves_bytes, uint64_t chunk_size,
                            uint64_t size) {
  if (chunk_size == 0) throw std::runtime_error(std::string(who) + ": chunk_size is 0");
  if (leaves_bytes % 32)
    throw std::runtime_error(std::string(who) + ": leaves length " +
                             std::to_string(leaves_bytes) + " is not a multiple of 32");
  uint64_t want = expected_leaf_count(size, chunk_size);
  if (leaves_bytes / 32 != want || want > UINT32_MAX)
    throw std::runtime_error(std::string(who) + ": " + std::to_string(leaves_bytes / 32) +
                             " leaves for " + std::to_string(size) + " bytes at chunk size " +
                             std::to_string(chunk_size) + " (expected " +
                             std::to_string(want) + ")");
  return static_cast<uint32_t>(want);
}

// What tar_index returns, from the engine and from the host model alike.
py::list indexed_files_to_py(const std::vector<tarhost::IndexedFile>& files) {
  py::list out;
  for (const tarhost::IndexedFile& f : files) {
    py::dict e;
    e["name"] = f.name;
    e["offset"] = f.offset;
    e["size"] = f.size;
    e["mode"] = f.mode;
    out.append(std::move(e));
  }
  return out;
}

struct Slot {
  char* host = nullptr;     // pinned
  hipEvent_t event = nullptr;
  size_t bytes = 0;
};

struct Range {
  uint64_t offset;
  uint64_t length;
};

// Owner of one hipMalloc'd allocation (move-only); the only place device
// memory is freed. Used directly for per-call temporaries.
class DeviceBuffer {
 public:
  DeviceBuffer() = default;
  explicit DeviceBuffer(size_t bytes) { HIP_CHECK(hipMalloc(&p_, bytes)); }
  DeviceBuffer(DeviceBuffer&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
    std::swap(p_, o.p_);
    return *this;
  }
  ~DeviceBuffer() {
    if (p_) hipFree(p_);
  }
  template <class T = void>
  T* get() const { return static_cast<T*>(p_); }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  void* p_ = nullptr;
};

// Grow-only device scratch kept across calls: per-call hipMalloc/hipFree of
// GiB-scale scratch dominated concurrent decompress (config-5 profile)
// before this. reserve() reallocates only when the request outgrows the
// capacity (contents are not carried over) and returns the buffer.
class DeviceScratch {
 public:
  template <class T = void>
  T* reserve(size_t bytes) {
    if (cap_ < bytes) {
      cap_ = 0;
      buf_ = DeviceBuffer();  // free first: old and new never coexist
      buf_ = DeviceBuffer(bytes);
      cap_ = bytes;
    }
    return buf_.get<T>();
  }

 private:
  DeviceBuffer buf_;
  size_t cap_ = 0;
};

// Keep-alive connection pool: checkout/checkin per (host,port). Reused
// sockets skip TCP connect + slow-start on every blob of an index — the
// per-blob latency term that dominates many-small-blob pulls (config 5).
class ConnPool {
 public:
  std::unique_ptr<http::ClientConn> checkout(const std::string& host, int port, bool tls) {
    std::lock_guard<std::mutex> lk(mu_);
    auto& v = pool_[(tls ? "https:" : "http:") + host + ":" + std::to_string(port)];
    if (!v.empty()) {
      auto c = std::move(v.back());
      v.pop_back();
      return c;
    }
    return std::make_unique<http::ClientConn>(host, port, tls);
  }
  void checkin(std::unique_ptr<http::ClientConn> c) {
    if (!c || !c->connected()) return;  // drop broken conns
    std::lock_guard<std::mutex> lk(mu_);
    auto& v = pool_[(c->tls() ? "https:" : "http:") + c->host() + ":" +
                    std::to_string(c->port())];
    if (v.size() < 64) v.push_back(std::move(c));
  }

 private:
  std::mutex mu_;
  std::map<std::string, std::vector<std::unique_ptr<http::ClientConn>>> pool_;
};

class GpuEngine {
 public:
  GpuEngine(int device, int num_slots, size_t slot_bytes, int num_streams)
      : device_(device), slot_bytes_(slot_bytes) {
    HIP_CHECK(hipSetDevice(device_));
    slots_.resize(num_slots);
    for (auto& s : slots_) {
      HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&s.host), slot_bytes,
                              hipHostMallocDefault));
      HIP_CHECK(hipEventCreateWithFlags(&s.event, hipEventDisableTiming));
      free_.push(&s);
    }
    streams_.resize(num_streams);
    for (auto& st : streams_) HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    HIP_CHECK(hipStreamCreateWithFlags(&hash_stream_, hipStreamNonBlocking));
    HIP_CHECK(hipEventCreateWithFlags(&zs_staged_, hipEventDisableTiming));
  }

  ~GpuEngine() {
    for (auto& st : streams_) hipStreamDestroy(st);
    hipStreamDestroy(hash_stream_);
    hipEventDestroy(zs_staged_);
    for (auto& s : slots_) {
      if (s.event) hipEventDestroy(s.event);
      if (s.host) hipHostFree(s.host);
    }
  }

  // ------------------------------------------------------------- pull ----

  // Download `size` bytes from `url` (plus optional extra headers) into the
  // device buffer at dst_ptr using ranged GETs on num_conns connections.
  // Returns timing stats.
  py::dict pull_to_device(const std::string& url,
                          const std::map<std::string, std::string>& headers, uint64_t size,
                          uintptr_t dst_ptr, int num_conns, uint64_t base_offset = 0) {
    std::string leaves;
    return pull_impl(url, headers, size, dst_ptr, num_conns, base_offset, 0, &leaves, nullptr);
  }

  // Fetch an explicit set of (offset, length) byte ranges of one object in
  // a single engine pass (shared connection workers + pinned ring) — the
  // chunk-dedup / chunk-refetch path, where spinning up the full pull
  // machinery per contiguous range would dominate.
  py::dict pull_ranges_to_device(const std::string& url,
                                 const std::map<std::string, std::string>& headers,
                                 const std::vector<std::pair<uint64_t, uint64_t>>& ranges,
                                 uintptr_t dst_ptr, int num_conns) {
    std::string leaves;
    std::vector<Range> rs;
    uint64_t total = 0;
    for (auto& r : ranges) {
      for (uint64_t off = 0; off < r.second; off += slot_bytes_)
        rs.push_back({r.first + off, std::min<uint64_t>(slot_bytes_, r.second - off)});
      total += r.second;
    }
    return pull_impl(url, headers, total, dst_ptr, num_conns, 0, 0, &leaves, &rs);
  }

  // Same, but ALSO hashes every landed slot with the CDNA4 SHA-256 chunk
  // kernel on the slot's own stream right after its H2D copy — verification
  // overlaps the remaining transfer ("verify as chunks land"). Returns
  // (stats, leaves). slot_bytes must be a chunk_size multiple (64 MiB / 128
  // KiB is), so every slot covers whole chunks.
  py::tuple pull_to_device_hashed(const std::string& url,
                                  const std::map<std::string, std::string>& headers,
                                  uint64_t size, uintptr_t dst_ptr, int num_conns,
                                  uint64_t chunk_size) {
    std::string leaves;
    py::dict stats =
        pull_impl(url, headers, size, dst_ptr, num_conns, 0, chunk_size, &leaves, nullptr);
    return py::make_tuple(stats, py::bytes(leaves));
  }

  py::dict pull_impl(const std::string& url, const std::map<std::string, std::string>& headers,
                     uint64_t size, uintptr_t dst_ptr, int num_conns, uint64_t base_offset,
                     uint64_t hash_chunk, std::string* leaves_out,
                     const std::vector<Range>* explicit_ranges) {
    DeviceBuffer dleaves;
    uint32_t total_chunks = 0;
    if (hash_chunk) {
      if (slot_bytes_ % hash_chunk != 0)
        throw std::runtime_error("slot_bytes must be a multiple of chunk_size");
      total_chunks = size ? static_cast<uint32_t>((size + hash_chunk - 1) / hash_chunk) : 1;
      dleaves = DeviceBuffer(static_cast<size_t>(total_chunks) * 32);
    }
    py::gil_scoped_release release;
    HIP_CHECK(hipSetDevice(device_));
    double t0 = now_s();

    // per-call pull state: pull_impl is reentrant — concurrent pulls (e.g.
    // many small blobs of one index from a Python thread pool) share the
    // pinned-slot pool and streams but own their range queue and error.
    // one HTTP request covers several pinned slots ("super-range"): the
    // response streams into consecutive slots, quartering per-request
    // overhead (headers, server sendfile setup) on big pulls. Explicit
    // range lists (dedup/refetch) are used as given.
    constexpr uint64_t kSlotsPerRequest = 4;
    std::vector<Range> ranges;
    if (explicit_ranges) {
      ranges = *explicit_ranges;
    } else {
      uint64_t super = slot_bytes_ * kSlotsPerRequest;
      for (uint64_t off = 0; off < size; off += super)
        ranges.push_back({off, std::min<uint64_t>(super, size - off)});
    }
    std::atomic<size_t> next_range{0};
    std::mutex err_mu;
    std::string error;
    std::atomic<uint64_t> net_bytes{0};
    std::atomic<long> net_ns{0};

    // reclaimer: waits for H2D events, returns slots to the free pool
    std::atomic<bool> done_submitting{false};
    std::thread reclaimer([&] {
      while (true) {
        Slot* s = nullptr;
        {
          std::unique_lock<std::mutex> lk(mu_);
          cv_pending_.wait(lk, [&] {
            return !pending_.empty() || (done_submitting.load() && pending_.empty());
          });
          if (pending_.empty()) break;
          s = pending_.front();
          pending_.pop_front();
        }
        hipEventSynchronize(s->event);
        {
          std::lock_guard<std::mutex> lk(mu_);
          free_.push(s);
        }
        cv_free_.notify_all();
      }
    });

    http::Url u = http::Url::parse(url);
    std::vector<std::thread> workers;
    std::atomic<int> stream_rr{0};
    for (int w = 0; w < num_conns; w++) {
      workers.emplace_back([&, w] {
        // no HIP_CHECK here: a throw out of a thread body is std::terminate
        if (hipError_t e = hipSetDevice(device_); e != hipSuccess) {
          std::lock_guard<std::mutex> lk(err_mu);
          if (error.empty()) error = std::string("hip: ") + hipGetErrorString(e);
          return;
        }
        auto conn_holder = conn_pool_.checkout(u.host, u.port, u.scheme == "https");
        http::ClientConn& conn = *conn_holder;
        http::Headers h;
        for (auto& kv : headers) h[kv.first] = kv.second;
        while (true) {
          Range r;
          {
            size_t i = next_range.fetch_add(1);
            if (i >= ranges.size()) break;
            {
              std::lock_guard<std::mutex> lk(err_mu);
              if (!error.empty()) break;
            }
            r = ranges[i];
          }
          // fetch the whole super-range in one request, landing each
          // slot-sized piece as it streams in; on failure retry the whole
          // super-range on a fresh connection (pieces are idempotent)
          bool ok = false;
          for (int attempt = 0; attempt < 3 && !ok; attempt++) {
            double tn = now_s();
            if (!begin_range_fetch(conn, u, h, {r.offset + base_offset, r.length})) continue;
            ok = true;
            for (uint64_t poff = 0; poff < r.length && ok; poff += slot_bytes_) {
              uint64_t plen = std::min<uint64_t>(slot_bytes_, r.length - poff);
              Slot* slot = acquire_slot();
              if (!conn.read_body_exact(slot->host, plen)) {
                conn.close_fd();
                release_slot(slot);
                ok = false;
                break;
              }
              uint64_t abs_off = r.offset + poff;
              hipStream_t st = streams_[stream_rr.fetch_add(1) % streams_.size()];
              hipError_t e = hipMemcpyAsync(reinterpret_cast<char*>(dst_ptr) + abs_off,
                                            slot->host, plen, hipMemcpyHostToDevice, st);
              if (e == hipSuccess && hash_chunk) {
                uint32_t first_chunk = static_cast<uint32_t>(abs_off / hash_chunk);
                uint32_t n_chunks =
                    static_cast<uint32_t>((plen + hash_chunk - 1) / hash_chunk);
                e = modelx_sha256_chunk_leaves(
                    reinterpret_cast<char*>(dst_ptr) + abs_off, plen, hash_chunk,
                    dleaves.get<char>() + static_cast<size_t>(first_chunk) * 32,
                    n_chunks, st);
              }
              if (e == hipSuccess) e = hipEventRecord(slot->event, st);
              if (e != hipSuccess) {
                {
                  std::lock_guard<std::mutex> lk(err_mu);
                  if (error.empty()) error = std::string("hip: ") + hipGetErrorString(e);
                }
                release_slot(slot);
                ok = false;
                // HIP errors are not retryable
                attempt = 3;
                break;
              }
              {
                std::lock_guard<std::mutex> lk(mu_);
                pending_.push_back(slot);
              }
              cv_pending_.notify_all();
            }
            if (ok) {
              net_ns.fetch_add(static_cast<long>((now_s() - tn) * 1e9));
              net_bytes.fetch_add(r.length);
            }
          }
          if (!ok) {
            std::lock_guard<std::mutex> lk(err_mu);
            if (error.empty()) error = "range fetch failed @" + std::to_string(r.offset);
            break;
          }
        }
        conn_pool_.checkin(std::move(conn_holder));
      });
    }
    for (auto& t : workers) t.join();
    done_submitting.store(true);
    cv_pending_.notify_all();
    reclaimer.join();
    for (auto& st : streams_) HIP_CHECK(hipStreamSynchronize(st));
    if (hash_chunk) {
      leaves_out->resize(static_cast<size_t>(total_chunks) * 32);
      HIP_CHECK(hipMemcpy(&(*leaves_out)[0], dleaves.get(), leaves_out->size(),
                          hipMemcpyDeviceToHost));
      // released here on success, not at scope exit: hipFree waits for the
      // device, and at scope exit the GIL is held again
      dleaves = DeviceBuffer();
    }
    double t1 = now_s();
    {
      std::lock_guard<std::mutex> lk(err_mu);
      if (!error.empty()) throw std::runtime_error("pull_to_device: " + error);
    }
    py::gil_scoped_acquire acquire;
    py::dict stats;
    stats["seconds"] = t1 - t0;
    stats["bytes"] = size;
    stats["gib_per_s"] = size / (t1 - t0) / (1 << 30);
    stats["net_conn_seconds"] = net_ns.load() / 1e9;
    return stats;
  }

  // -------------------------------------------------------------- hash ----

  // Chunked-digest leaves of a device buffer; returns leaves as bytes.
  py::bytes sha256_chunk_leaves(uintptr_t dev_ptr, uint64_t size, uint64_t chunk_size) {
    if (chunk_size == 0) throw std::runtime_error("sha256_chunk_leaves: chunk_size is 0");
    HIP_CHECK(hipSetDevice(device_));
    uint32_t nchunks = static_cast<uint32_t>(expected_leaf_count(size, chunk_size));
    std::string out;
    {
      // temporaries live inside the GIL-released block: hipFree waits for
      // the device and must not do so holding the GIL
      py::gil_scoped_release release;
      DeviceBuffer dleaves(static_cast<size_t>(nchunks) * 32);
      HIP_CHECK(modelx_sha256_chunk_leaves(reinterpret_cast<void*>(dev_ptr), size, chunk_size,
                                           dleaves.get(), nchunks, hash_stream_));
      out.resize(static_cast<size_t>(nchunks) * 32);
      HIP_CHECK(hipStreamSynchronize(hash_stream_));
      HIP_CHECK(hipMemcpy(&out[0], dleaves.get(), out.size(), hipMemcpyDeviceToHost));
    }
    return py::bytes(out);
  }

  // Canonical sha256 of N device buffers (ptr,len) — batched, one per lane.
  py::bytes sha256_multibuf(const std::vector<std::pair<uintptr_t, uint64_t>>& bufs) {
    HIP_CHECK(hipSetDevice(device_));
    uint32_t n = static_cast<uint32_t>(bufs.size());
    if (n == 0) return py::bytes("");
    std::vector<const void*> hptrs(n);
    std::vector<uint64_t> hlens(n);
    for (uint32_t i = 0; i < n; i++) {
      hptrs[i] = reinterpret_cast<const void*>(bufs[i].first);
      hlens[i] = bufs[i].second;
    }
    std::string out;
    {
      py::gil_scoped_release release;
      DeviceBuffer dptrs(n * sizeof(void*));
      DeviceBuffer dlens(n * sizeof(uint64_t));
      DeviceBuffer ddig(static_cast<size_t>(n) * 32);
      // stream-ordered staging: a plain hipMemcpy is NOT ordered against a
      // kernel launched on a non-blocking stream — the kernel could read
      // stale parameters (observed as rare packed-frame corruption in the
      // equivalent zstd path)
      HIP_CHECK(hipMemcpyAsync(dptrs.get(), hptrs.data(), n * sizeof(void*),
                               hipMemcpyHostToDevice, hash_stream_));
      HIP_CHECK(hipMemcpyAsync(dlens.get(), hlens.data(), n * sizeof(uint64_t),
                               hipMemcpyHostToDevice, hash_stream_));
      HIP_CHECK(modelx_sha256_multibuf(dptrs.get<const void*>(), dlens.get<uint64_t>(), n,
                                       ddig.get(), hash_stream_));
      out.resize(static_cast<size_t>(n) * 32);
      HIP_CHECK(hipStreamSynchronize(hash_stream_));
      HIP_CHECK(hipMemcpy(&out[0], ddig.get(), out.size(), hipMemcpyDeviceToHost));
    }
    return py::bytes(out);
  }

  // Bounded D2H read of device memory (registry-stream push fallback:
  // slot-sized pieces fed to a streaming HTTP PUT).
  py::bytes read_device(uintptr_t src_ptr, uint64_t size) {
    HIP_CHECK(hipSetDevice(device_));
    std::string out(size, '\0');
    {
      py::gil_scoped_release release;
      HIP_CHECK(hipMemcpy(&out[0], reinterpret_cast<void*>(src_ptr), size,
                          hipMemcpyDeviceToHost));
    }
    return py::bytes(out);
  }

  // Canonical (wire-compatible) byte-stream SHA-256 of device memory.
  // Plain SHA-256 is strictly sequential at 64 B granularity, so a GPU lane
  // is ~4× SLOWER than a SHA-NI CPU core for a single chain — the right
  // MI355X split is: stream the bytes D2H through the pinned ring
  // (double-buffered, overlapped) and run the one sequential chain on the
  // CPU's SHA-NI units (OpenSSL EVP, ~2 GiB/s/core). Multi-blob pushes get
  // their parallelism across blobs (one call per blob from a thread pool —
  // the GIL is released for the whole call). Reference semantics:
  // pkg/client/push.go:149-161 (go-digest streaming sha256).
  py::bytes sha256_canonical_device(uintptr_t src_ptr, uint64_t size) {
    HIP_CHECK(hipSetDevice(device_));
    unsigned char md[32];
    {
      py::gil_scoped_release release;
      std::unique_ptr<EVP_MD_CTX, decltype(&EVP_MD_CTX_free)> ctx(EVP_MD_CTX_new(),
                                                                  &EVP_MD_CTX_free);
      if (!ctx || EVP_DigestInit_ex(ctx.get(), EVP_sha256(), nullptr) != 1)
        throw std::runtime_error("EVP sha256 init failed");
      hipError_t e = drain_device(src_ptr, size, [&](const char* p, uint64_t len) {
        EVP_DigestUpdate(ctx.get(), p, len);
        return true;
      });
      if (e != hipSuccess)
        throw std::runtime_error(std::string("sha256_canonical_device: hip: ") +
                                 hipGetErrorString(e));
      unsigned int mdlen = 0;
      EVP_DigestFinal_ex(ctx.get(), md, &mdlen);
    }
    return py::bytes(reinterpret_cast<char*>(md), 32);
  }

  // -------------------------------------------------------------- push ----

  // Upload device memory [src_ptr, src_ptr+size) as the body of `method` to
  // url (one part). Streams D2H through the pinned ring. The pooled
  // connection goes back to the pool only once the response has been read;
  // every failure path simply drops it.
  py::dict push_part_from_device(const std::string& url, const std::string& method,
                                 const std::map<std::string, std::string>& headers,
                                 uintptr_t src_ptr, uint64_t size) {
    py::gil_scoped_release release;
    HIP_CHECK(hipSetDevice(device_));
    double t0 = now_s();
    http::Url u = http::Url::parse(url);
    auto conn_holder = conn_pool_.checkout(u.host, u.port, u.scheme == "https");
    http::ClientConn& conn = *conn_holder;
    http::Headers h;
    for (auto& kv : headers) h[kv.first] = kv.second;
    if (!conn.send_request(method, u.target(), h, static_cast<int64_t>(size)))
      throw std::runtime_error("push: send_request failed");
    bool sent = true;
    HIP_CHECK(drain_device(src_ptr, size, [&](const char* p, uint64_t len) {
      return sent = conn.send_body(p, len);
    }));
    if (!sent) throw std::runtime_error("push: send_body failed");
    int status = 0;
    http::Headers rh;
    if (!conn.read_response_head(&status, &rh)) throw std::runtime_error("push: no response");
    char drain[4096];
    while (conn.read_body(drain, sizeof drain) > 0) {
    }
    conn_pool_.checkin(std::move(conn_holder));
    double t1 = now_s();
    if (status < 200 || status >= 300)
      throw std::runtime_error("push: HTTP " + std::to_string(status));
    py::gil_scoped_acquire acquire;
    py::dict stats;
    stats["seconds"] = t1 - t0;
    stats["bytes"] = size;
    stats["status"] = status;
    return stats;
  }

  // ---------------------------------------------------- tar (directories) --

  // Index a tar archive resident in HBM: [{name, offset, size, mode}] for
  // its regular files, as tarfile lists them. The header walk runs on the
  // device (tar_core.hpp's, the one _core.tar_index_host runs on host
  // bytes), the scatter kernel gathers the header blocks for one D2H copy,
  // and tar_host.hpp checks the table against tar_len and resolves the
  // names. A damaged or unsupported archive is a RuntimeError naming the
  // cause and the header offset; no payload byte is read before the whole
  // table has passed the host-side check.
  py::list tar_index(uintptr_t tar_ptr, uint64_t tar_len) {
    HIP_CHECK(hipSetDevice(device_));
    uint32_t max_entries = tarhost::kMaxIndexEntries;  // tar_pack emits no more
    std::vector<TarEntry> entries;
    std::string headers;
    {
      py::gil_scoped_release release;
      DeviceBuffer dentries(max_entries * sizeof(TarEntry));
      DeviceBuffer dresult(sizeof(TarWalkResult));
      HIP_CHECK(modelx_tar_index(reinterpret_cast<void*>(tar_ptr), tar_len,
                                 dentries.get<TarEntry>(), max_entries,
                                 dresult.get<TarWalkResult>(), hash_stream_));
      HIP_CHECK(hipStreamSynchronize(hash_stream_));
      TarWalkResult res;
      HIP_CHECK(hipMemcpy(&res, dresult.get(), sizeof res, hipMemcpyDeviceToHost));
      if (res.error) throw tarhost::IndexError(res.error, res.error_off);
      if (res.count > max_entries)
        throw tarhost::IndexError(tarcore::kErrTooManyEntries, 0);
      entries.resize(res.count);
      if (res.count)
        HIP_CHECK(hipMemcpy(entries.data(), dentries.get(), res.count * sizeof(TarEntry),
                            hipMemcpyDeviceToHost));
      // before the gather below reads a header by these offsets
      tarhost::validate_entries(entries, tar_len);
      // gather the header blocks to the host in one shot
      headers.assign(entries.size() * tarhost::kBlock, '\0');
      if (!entries.empty()) {
        DeviceBuffer dgather(headers.size());
        std::vector<CopySeg> segs(entries.size());
        for (size_t i = 0; i < entries.size(); i++)
          segs[i] = {entries[i].header_off,
                     reinterpret_cast<uint64_t>(dgather.get()) + i * tarhost::kBlock,
                     tarhost::kBlock};
        DeviceBuffer dsegs(segs.size() * sizeof(CopySeg));
        HIP_CHECK(hipMemcpyAsync(dsegs.get(), segs.data(), segs.size() * sizeof(CopySeg),
                                 hipMemcpyHostToDevice, hash_stream_));
        HIP_CHECK(modelx_tar_scatter(reinterpret_cast<void*>(tar_ptr), dsegs.get<CopySeg>(),
                                     static_cast<uint32_t>(segs.size()), hash_stream_));
        HIP_CHECK(hipStreamSynchronize(hash_stream_));
        HIP_CHECK(hipMemcpy(&headers[0], dgather.get(), headers.size(), hipMemcpyDeviceToHost));
      }
    }
    // payloads of 'L', 'x' and 'g' entries; resolve_names validates the
    // table against tar_len before its first call
    auto read_payload = [&](const TarEntry& e) {
      std::string pl(static_cast<size_t>(e.size), '\0');
      if (!pl.empty())
        HIP_CHECK(hipMemcpy(&pl[0], reinterpret_cast<char*>(tar_ptr) + e.payload_off, pl.size(),
                            hipMemcpyDeviceToHost));
      return pl;
    };
    std::vector<tarhost::IndexedFile> files;
    {
      py::gil_scoped_release release;
      files = tarhost::resolve_names(entries, headers.data(), read_payload, tar_len);
    }
    return indexed_files_to_py(files);
  }

  // Scatter payload segments: [(src_off, dst_dev_ptr, len), ...]
  void tar_scatter(uintptr_t tar_ptr,
                   const std::vector<std::tuple<uint64_t, uintptr_t, uint64_t>>& segs) {
    HIP_CHECK(hipSetDevice(device_));
    if (segs.empty()) return;
    py::gil_scoped_release release;
    // split into <=4 MiB pieces for load balance across CUs
    std::vector<CopySeg> pieces;
    constexpr uint64_t kPiece = 4ull << 20;
    for (auto& t : segs) {
      uint64_t src_off = std::get<0>(t), dst = std::get<1>(t), len = std::get<2>(t);
      for (uint64_t off = 0; off < len; off += kPiece)
        pieces.push_back({src_off + off, dst + off, std::min(kPiece, len - off)});
    }
    if (pieces.empty()) return;  // zero-length segments only
    DeviceBuffer dsegs(pieces.size() * sizeof(CopySeg));
    HIP_CHECK(hipMemcpyAsync(dsegs.get(), pieces.data(), pieces.size() * sizeof(CopySeg),
                             hipMemcpyHostToDevice, hash_stream_));
    HIP_CHECK(modelx_tar_scatter(reinterpret_cast<void*>(tar_ptr), dsegs.get<CopySeg>(),
                                 static_cast<uint32_t>(pieces.size()), hash_stream_));
    HIP_CHECK(hipStreamSynchronize(hash_stream_));
  }

  // Pack device buffers into one plain-tar archive at dst_ptr (device):
  // members = [(name, src_dev_ptr, size), ...] in archive order. The layout
  // and header bytes come from tar_host.hpp; the kernel writes every byte of
  // [0, total) — headers, payload pieces, 512 B padding and the end marker —
  // so the destination needs no memset. Returns total.
  uint64_t tar_pack(uintptr_t dst_ptr, uint64_t dst_cap,
                    const std::vector<std::tuple<std::string, uintptr_t, uint64_t>>& members) {
    std::vector<std::pair<std::string, uint64_t>> names;
    names.reserve(members.size());
    for (auto& m : members) names.emplace_back(std::get<0>(m), std::get<2>(m));
    tarhost::PackLayout lay = tarhost::pack_layout(names);
    if (lay.total > dst_cap)
      throw std::runtime_error("tar_pack: archive of " + std::to_string(lay.total) +
                               " bytes exceeds destination capacity " +
                               std::to_string(dst_cap));
    if (dst_ptr & 15u) throw std::runtime_error("tar_pack: destination is not 16-byte aligned");
    HIP_CHECK(hipSetDevice(device_));
    py::gil_scoped_release release;
    DeviceBuffer dheaders(std::max<size_t>(lay.headers.size(), 1));
    uint64_t hbase = reinterpret_cast<uint64_t>(dheaders.get());
    // header regions, then payloads in <=4 MiB pieces (the last one carries
    // the zero padding up to the 512 B boundary), then the end marker
    std::vector<PackSeg> segs;
    constexpr uint64_t kPiece = 4ull << 20;
    uint64_t hoff = 0;
    for (size_t i = 0; i < members.size(); i++) {
      const tarhost::PackEntry& e = lay.entries[i];
      segs.push_back({hbase + hoff, e.header_off, e.header_len, 0});
      hoff += e.header_len;
      uint64_t src = std::get<1>(members[i]);
      for (uint64_t off = 0; off < e.size; off += kPiece) {
        uint64_t len = std::min(kPiece, e.size - off);
        bool last = off + len == e.size;
        segs.push_back({src + off, e.payload_off + off, len,
                        last ? tarhost::pad512(e.size) - e.size : 0});
      }
    }
    segs.push_back({0, lay.total - 2 * tarhost::kBlock, 0, 2 * tarhost::kBlock});
    DeviceBuffer dsegs(segs.size() * sizeof(PackSeg));
    if (!lay.headers.empty())
      HIP_CHECK(hipMemcpyAsync(dheaders.get(), lay.headers.data(), lay.headers.size(),
                               hipMemcpyHostToDevice, hash_stream_));
    HIP_CHECK(hipMemcpyAsync(dsegs.get(), segs.data(), segs.size() * sizeof(PackSeg),
                             hipMemcpyHostToDevice, hash_stream_));
    HIP_CHECK(modelx_tar_pack(reinterpret_cast<void*>(dst_ptr), dsegs.get<PackSeg>(),
                              static_cast<uint32_t>(segs.size()), hash_stream_));
    HIP_CHECK(hipStreamSynchronize(hash_stream_));
    return lay.total;
  }

  // ------------------------------------------------------ byte planes ----

  // Byte-plane split (merge=false) or merge (merge=true) of device buffers
  // (core/hip/byteplane.hip; the transform is byteplane_host.hpp's).
  // items = [(src_ptr, dst_ptr, size, elem, group)]. Every item is checked
  // before the first launch; then all launch on hash_stream_ with ONE sync
  // (the batching rule of zstd_decompress_many). size == 0 is a no-op.
  void byte_planes(
      const std::vector<std::tuple<uintptr_t, uintptr_t, uint64_t, uint64_t, uint64_t>>& items,
      bool merge) {
    for (size_t i = 0; i < items.size(); i++) {
      auto [src, dst, size, elem, group] = items[i];
      try {
        byteplane::validate(elem, group);
      } catch (const std::invalid_argument& e) {
        throw std::runtime_error(std::string(e.what()) + " (item " + std::to_string(i) + ")");
      }
      if (size == 0) continue;
      if (src > UINTPTR_MAX - size || dst > UINTPTR_MAX - size)
        throw std::runtime_error("byte planes: item " + std::to_string(i) +
                                 " wraps the address space");
      if (src < dst + size && dst < src + size)
        throw std::runtime_error("byte planes: source and destination of item " +
                                 std::to_string(i) + " overlap");
    }
    HIP_CHECK(hipSetDevice(device_));
    py::gil_scoped_release release;
    bool launched = false;
    for (auto& [src, dst, size, elem, group] : items) {
      if (size == 0) continue;
      HIP_CHECK(modelx_byte_planes(reinterpret_cast<const void*>(src),
                                   reinterpret_cast<void*>(dst), size,
                                   static_cast<uint32_t>(elem), group, merge ? 1 : 0,
                                   hash_stream_));
      launched = true;
    }
    if (launched) HIP_CHECK(hipStreamSynchronize(hash_stream_));
  }

  // ------------------------------------------------------------- zstd ----

  // Compress a device buffer into a seekable multi-frame zstd blob at
  // dst_ptr (device). Returns the total blob size (frames + seek table).
  // One workgroup per frame (core/hip/zstd.hip); frames are compressed into
  // padded per-frame scratch in batches, packed with the scatter kernel,
  // and the seek table is appended from the host. literals_only skips the LZ
  // parse (EncTables::flags bit 2): right for byte planes of dense float
  // data, worse on mostly-zero data, where Huffman cannot go below one bit
  // per byte.
  uint64_t zstd_compress_device(uintptr_t src_ptr, uint64_t size, uint32_t frame_raw,
                                uintptr_t dst_ptr, uint64_t dst_cap, bool literals_only) {
    HIP_CHECK(hipSetDevice(device_));
    const uint32_t flags = zstd_flags() | (literals_only ? zstd::kEncLiteralsOnly : 0u);
    if (frame_raw == 0) frame_raw = 128 << 10;
    using namespace modelx::zstd;
    uint64_t nframes = size ? (size + frame_raw - 1) / frame_raw : 1;
    uint64_t stride = (uint64_t)frame_raw + 64 + 3 * ((frame_raw + kBlockMax - 1) / kBlockMax);
    uint32_t max_seqs = kBlockMax / 4 + 1;
    uint64_t batch = std::min<uint64_t>(nframes, 4096);
    std::vector<zstdhost::SeekEntry> entries(nframes);
    py::gil_scoped_release release;
    std::lock_guard<std::mutex> zlk(zstd_mu_);
    void* dscratch = zs_compress_.reserve(batch * stride);
    void* dseqs = zs_seqs_.reserve(batch * (uint64_t)max_seqs * 12);
    int64_t* dsizes = zs_sizes_.reserve<int64_t>(batch * sizeof(int64_t));
    CopySeg* dsegs = zs_segs_.reserve<CopySeg>(batch * sizeof(CopySeg));
    std::vector<int64_t> hsizes(batch);
    std::vector<CopySeg> hsegs(batch);
    uint64_t out = 0;
    for (uint64_t first = 0; first < nframes; first += batch) {
      uint32_t n = (uint32_t)std::min<uint64_t>(batch, nframes - first);
      HIP_CHECK(modelx_zstd_compress_frames(reinterpret_cast<void*>(src_ptr), size, frame_raw,
                                            (uint32_t)first, n, dscratch, stride, dseqs,
                                            max_seqs, dsizes, flags, hash_stream_));
      HIP_CHECK(hipStreamSynchronize(hash_stream_));
      HIP_CHECK(hipMemcpy(hsizes.data(), dsizes, n * sizeof(int64_t), hipMemcpyDeviceToHost));
      for (uint32_t i = 0; i < n; i++) {
        if (hsizes[i] < 0)
          throw std::runtime_error("zstd compress kernel failed: frame " +
                                   std::to_string(first + i) + " rc=" +
                                   std::to_string(hsizes[i]));
        uint64_t f = first + i;
        uint64_t d_off = f * (uint64_t)frame_raw;
        entries[f] = {out, (uint64_t)hsizes[i], d_off,
                      std::min<uint64_t>(frame_raw, size - std::min(size, d_off))};
        if (size == 0) entries[f].d_size = 0;
        hsegs[i] = {i * stride, dst_ptr + out, (uint64_t)hsizes[i]};
        out += (uint64_t)hsizes[i];
        if (out > dst_cap) throw std::runtime_error("zstd compress: dst overflow");
      }
      HIP_CHECK(hipMemcpyAsync(dsegs, hsegs.data(), n * sizeof(CopySeg),
                               hipMemcpyHostToDevice, hash_stream_));
      HIP_CHECK(modelx_tar_scatter(dscratch, dsegs, n, hash_stream_));
      HIP_CHECK(hipStreamSynchronize(hash_stream_));
    }
    auto table = zstdhost::build_seek_table(entries);
    if (out + table.size() > dst_cap) throw std::runtime_error("zstd compress: dst overflow");
    HIP_CHECK(hipMemcpyAsync(reinterpret_cast<char*>(dst_ptr) + out, table.data(),
                             table.size(), hipMemcpyHostToDevice, hash_stream_));
    HIP_CHECK(hipStreamSynchronize(hash_stream_));
    out += table.size();
    return out;
  }

  // Decompress a seekable multi-frame zstd blob resident in HBM into
  // dst_ptr. Parses the seek table from the blob tail (one small D2H copy),
  // then decodes every frame in its own workgroup. Returns decompressed
  // size.
  uint64_t zstd_decompress_device(uintptr_t src_ptr, uint64_t src_len, uintptr_t dst_ptr,
                                  uint64_t dst_cap) {
    HIP_CHECK(hipSetDevice(device_));
    using namespace modelx::zstd;
    py::gil_scoped_release release;
    const char* src = reinterpret_cast<const char*>(src_ptr);
    // footer, then the table it describes; the format and every check that
    // keeps a corrupt blob's offsets from the kernel: zstdhost::parse_seek_*
    uint8_t foot[zstdhost::kSeekFooterBytes] = {};
    if (src_len >= sizeof foot)  // a shorter blob is rejected by the parser
      HIP_CHECK(hipMemcpy(foot, src + src_len - sizeof foot, sizeof foot, hipMemcpyDeviceToHost));
    zstdhost::SeekFooter ft = zstdhost::parse_seek_footer(foot, src_len);
    std::vector<uint8_t> traw(ft.table_bytes);
    HIP_CHECK(hipMemcpy(traw.data(), src + src_len - ft.table_bytes, ft.table_bytes,
                        hipMemcpyDeviceToHost));
    std::vector<SeekEntry> frames;
    uint64_t d_total = zstdhost::parse_seek_entries(traw.data(), ft, src_len, &frames);
    if (d_total > dst_cap) throw std::runtime_error("zstd decompress: dst too small");
    uint64_t nframes = frames.size();
    uint64_t batch = std::min<uint64_t>(nframes ? nframes : 1, 8192);
    std::lock_guard<std::mutex> zlk(zstd_mu_);
    SeekEntry* dframes = zs_frames_.reserve<SeekEntry>(batch * sizeof(SeekEntry));
    void* dlit = zs_lit_.reserve(batch * (uint64_t)kBlockMax);
    int64_t* drc = zs_rc_.reserve<int64_t>(batch * sizeof(int64_t));
    std::vector<int64_t> hrc(batch);
    for (uint64_t first = 0; first < nframes; first += batch) {
      uint32_t n = (uint32_t)std::min<uint64_t>(batch, nframes - first);
      HIP_CHECK(hipMemcpyAsync(dframes, frames.data() + first, n * sizeof(SeekEntry),
                               hipMemcpyHostToDevice, hash_stream_));
      HIP_CHECK(modelx_zstd_decompress_frames(src, dframes, n, reinterpret_cast<void*>(dst_ptr),
                                              dlit, drc, zstd_flags(), hash_stream_));
      HIP_CHECK(hipStreamSynchronize(hash_stream_));
      HIP_CHECK(hipMemcpy(hrc.data(), drc, n * sizeof(int64_t), hipMemcpyDeviceToHost));
      for (uint32_t i = 0; i < n; i++)
        if (hrc[i] != 0)
          throw std::runtime_error("zstd decompress kernel failed: frame " +
                                   std::to_string(first + i) + " rc=" + std::to_string(hrc[i]));
    }
    return d_total;
  }

  // Batched decode of MANY seekable blobs in one call. The single-blob
  // path costs ~5 stream round-trips per blob (footer, table, batch sync,
  // rc check) serialized under zstd_mu_ — measured 4.1 GiB/s effective on
  // config-5's 64 MiB blobs against a 240-540 GiB/s kernel. Here the
  // footer/table parses collapse to two syncs for the whole set, decode
  // launches spread across the engine streams, and ONE final sync checks
  // every frame's rc. items = [(src_ptr, src_len, dst_ptr, dst_cap)];
  // returns decompressed sizes.
  std::vector<uint64_t> zstd_decompress_many(
      const std::vector<std::tuple<uintptr_t, uint64_t, uintptr_t, uint64_t>>& items) {
    HIP_CHECK(hipSetDevice(device_));
    using namespace modelx::zstd;
    constexpr size_t kFoot = zstdhost::kSeekFooterBytes;
    size_t n = items.size();
    std::vector<uint64_t> out(n, 0);
    if (!n) return out;
    auto src_of = [&](size_t i) { return reinterpret_cast<const char*>(std::get<0>(items[i])); };
    auto len_of = [&](size_t i) { return std::get<1>(items[i]); };
    py::gil_scoped_release release;
    std::lock_guard<std::mutex> zlk(zstd_mu_);
    // phase 1: all footers, one sync
    std::vector<uint8_t> foots(n * kFoot, 0);
    for (size_t i = 0; i < n; i++) {
      if (len_of(i) < kFoot) continue;  // rejected by the parser below
      HIP_CHECK(hipMemcpyAsync(foots.data() + i * kFoot, src_of(i) + len_of(i) - kFoot, kFoot,
                               hipMemcpyDeviceToHost, hash_stream_));
    }
    HIP_CHECK(hipStreamSynchronize(hash_stream_));
    std::vector<zstdhost::SeekFooter> foot(n);
    std::vector<uint64_t> tbl_off(n);
    uint64_t total_tbl = 0;
    for (size_t i = 0; i < n; i++) {
      foot[i] = zstdhost::parse_seek_footer(foots.data() + i * kFoot, len_of(i));
      tbl_off[i] = total_tbl;
      total_tbl += foot[i].table_bytes;
    }
    // phase 2: all tables, one sync
    std::vector<uint8_t> traw(total_tbl);
    for (size_t i = 0; i < n; i++)
      HIP_CHECK(hipMemcpyAsync(traw.data() + tbl_off[i],
                               src_of(i) + len_of(i) - foot[i].table_bytes,
                               foot[i].table_bytes, hipMemcpyDeviceToHost, hash_stream_));
    HIP_CHECK(hipStreamSynchronize(hash_stream_));
    std::vector<SeekEntry> frames;
    std::vector<std::pair<size_t, size_t>> item_span(n);  // [first, count) into frames
    uint64_t max_chunk = 1;
    for (size_t i = 0; i < n; i++) {
      size_t first = frames.size();
      out[i] = zstdhost::parse_seek_entries(traw.data() + tbl_off[i], foot[i], len_of(i),
                                            &frames);
      if (out[i] > std::get<3>(items[i]))
        throw std::runtime_error("zstd decompress: dst too small");
      item_span[i] = {first, frames.size() - first};
      max_chunk = std::max<uint64_t>(
          max_chunk, std::min<uint64_t>(foot[i].nframes ? foot[i].nframes : 1, 8192));
    }
    if (frames.empty()) return out;
    // phase 3: one frame-array H2D, decode launches across streams
    size_t ns = streams_.size();
    SeekEntry* dframes = zs_frames_.reserve<SeekEntry>(frames.size() * sizeof(SeekEntry));
    int64_t* drc = zs_rc_.reserve<int64_t>(frames.size() * sizeof(int64_t));
    char* dlit = zs_lit_.reserve<char>(ns * max_chunk * (uint64_t)kBlockMax);
    HIP_CHECK(hipMemcpyAsync(dframes, frames.data(), frames.size() * sizeof(SeekEntry),
                             hipMemcpyHostToDevice, hash_stream_));
    HIP_CHECK(hipEventRecord(zs_staged_, hash_stream_));
    for (size_t s = 0; s < ns; s++) HIP_CHECK(hipStreamWaitEvent(streams_[s], zs_staged_, 0));
    size_t rr = 0;
    for (size_t i = 0; i < n; i++) {
      auto [first, count] = item_span[i];
      for (size_t off = 0; off < count; off += max_chunk) {
        uint32_t nb = (uint32_t)std::min<uint64_t>(max_chunk, count - off);
        size_t sidx = rr++ % ns;
        HIP_CHECK(modelx_zstd_decompress_frames(
            src_of(i), dframes + first + off, nb,
            reinterpret_cast<void*>(std::get<2>(items[i])),
            dlit + sidx * max_chunk * (uint64_t)kBlockMax, drc + first + off, zstd_flags(),
            streams_[sidx]));
      }
    }
    for (auto& st : streams_) HIP_CHECK(hipStreamSynchronize(st));
    std::vector<int64_t> hrc(frames.size());
    HIP_CHECK(hipMemcpy(hrc.data(), drc, frames.size() * sizeof(int64_t),
                        hipMemcpyDeviceToHost));
    for (size_t f = 0; f < hrc.size(); f++)
      if (hrc[f] != 0)
        throw std::runtime_error("zstd decompress kernel failed: frame " + std::to_string(f) +
                                 " rc=" + std::to_string(hrc[f]));
    return out;
  }

  // Batched chunk-leaf digests of many device buffers: all launches on
  // hash_stream_, ONE sync, ONE D2H — the per-blob sha256_chunk_leaves
  // round trips were the other orchestration term on many-small-blob
  // indexes. items = [(ptr, size, chunk_size)].
  std::vector<py::bytes> sha256_chunk_leaves_many(
      const std::vector<std::tuple<uintptr_t, uint64_t, uint64_t>>& items) {
    HIP_CHECK(hipSetDevice(device_));
    size_t n = items.size();
    std::vector<py::bytes> res;
    if (!n) return res;
    std::vector<uint32_t> nchunks(n);
    std::vector<uint64_t> off(n);
    uint64_t total = 0;
    for (size_t i = 0; i < n; i++) {
      auto [ptr, size, cs] = items[i];
      (void)ptr;
      if (cs == 0)
        throw std::runtime_error("sha256_chunk_leaves_many: chunk_size is 0 (item " +
                                 std::to_string(i) + ")");
      nchunks[i] = (uint32_t)expected_leaf_count(size, cs);
      off[i] = total;
      total += nchunks[i];
    }
    std::string host;
    {
      py::gil_scoped_release release;
      std::lock_guard<std::mutex> zlk(zstd_mu_);
      char* dleaves = zs_leaves_.reserve<char>(total * 32);
      // ONE launch over all buffers: per-blob launches leave the chip
      // near-idle on small blobs (a 64 MiB blob is only 512 chains)
      std::vector<ChunkLeavesDesc> descs(n);
      for (size_t i = 0; i < n; i++) {
        auto [ptr, size, cs] = items[i];
        descs[i] = {reinterpret_cast<const uint8_t*>(ptr),
                    reinterpret_cast<uint8_t*>(dleaves + off[i] * 32), size, cs,
                    (uint32_t)off[i], 0};
      }
      ChunkLeavesDesc* ddescs = zs_descs_.reserve<ChunkLeavesDesc>(n * sizeof(ChunkLeavesDesc));
      HIP_CHECK(hipMemcpyAsync(ddescs, descs.data(), n * sizeof(ChunkLeavesDesc),
                               hipMemcpyHostToDevice, hash_stream_));
      HIP_CHECK(modelx_sha256_chunk_leaves_many(ddescs, (uint32_t)n, (uint32_t)total,
                                                hash_stream_));
      HIP_CHECK(hipStreamSynchronize(hash_stream_));
      host.resize(total * 32);
      HIP_CHECK(hipMemcpy(&host[0], dleaves, host.size(), hipMemcpyDeviceToHost));
    }
    for (size_t i = 0; i < n; i++)
      res.emplace_back(host.data() + off[i] * 32, (size_t)nchunks[i] * 32);
    return res;
  }

  // Upper bound for zstd_compress_device output.
  static uint64_t zstd_compress_bound(uint64_t size, uint32_t frame_raw) {
    using namespace modelx::zstd;
    if (frame_raw == 0) frame_raw = 128 << 10;
    uint64_t nframes = size ? (size + frame_raw - 1) / frame_raw : 1;
    uint64_t stride = (uint64_t)frame_raw + 64 + 3 * ((frame_raw + kBlockMax - 1) / kBlockMax);
    return nframes * stride + 8 + nframes * 8 + 9;
  }

  // ------------------------------------------------------ chunk dedup ----
  // HBM-resident chunk hash table (core/hip/dedup.hip). Insert/probe/gather
  // run on hash_stream_ under dedup_mu_; the caller (GpuClient) keeps the
  // registered tensors alive.

  void dedup_reset(uint64_t cap_pow2) {
    // the kernels mask with cap - 1 and probe a window of kDedupMaxProbes
    if (cap_pow2 && ((cap_pow2 & (cap_pow2 - 1)) || cap_pow2 < kDedupMaxProbes))
      throw std::runtime_error("dedup_reset: capacity " + std::to_string(cap_pow2) +
                               " is not a power of two >= " +
                               std::to_string(kDedupMaxProbes));
    HIP_CHECK(hipSetDevice(device_));
    py::gil_scoped_release release;
    std::lock_guard<std::mutex> lk(dedup_mu_);
    if (cap_pow2 == 0) cap_pow2 = dedup_cap_ ? dedup_cap_ : (1ull << 22);
    if (dedup_cap_ != cap_pow2) {
      dedup_cap_ = 0;
      dedup_table_ = DeviceBuffer();  // free first: old and new never coexist
      dedup_table_ = DeviceBuffer(cap_pow2 * 48);
      dedup_cap_ = cap_pow2;
    }
    if (!dedup_dropped_) dedup_dropped_ = DeviceBuffer(sizeof(uint32_t));
    HIP_CHECK(hipMemsetAsync(dedup_table_.get(), 0, dedup_cap_ * 48, hash_stream_));
    HIP_CHECK(hipMemsetAsync(dedup_dropped_.get(), 0, sizeof(uint32_t), hash_stream_));
    HIP_CHECK(hipStreamSynchronize(hash_stream_));
  }

  // Register a blob's chunks (leaves = packed 32 B digests, host bytes).
  // Returns the running dropped-entry count (table pressure indicator).
  uint32_t dedup_register(py::bytes leaves, uintptr_t base, uint64_t chunk_size,
                          uint64_t total) {
    std::string lv = leaves;
    uint32_t nleaves = checked_leaf_count("dedup_register", lv.size(), chunk_size, total);
    HIP_CHECK(hipSetDevice(device_));
    py::gil_scoped_release release;
    // Repeated leaves (zero-filled tensors, padding) are dropped here, first
    // index kept: every key of one insert launch is then distinct, so a
    // lane that loses the CAS never has to read the winner's payload to
    // recognise its own digest (see dedup.hip).
    std::string uniq;
    std::vector<uint32_t> idx;
    {
      std::unordered_set<std::string_view> seen;
      seen.reserve(nleaves);
      idx.reserve(nleaves);
      for (uint32_t i = 0; i < nleaves; i++)
        if (seen.insert(std::string_view(lv.data() + (size_t)i * 32, 32)).second)
          idx.push_back(i);
      uniq.reserve(idx.size() * 36);
      for (uint32_t i : idx) uniq.append(lv.data() + (size_t)i * 32, 32);
      uniq.append(reinterpret_cast<const char*>(idx.data()), idx.size() * 4);
    }
    uint32_t n = static_cast<uint32_t>(idx.size());
    std::lock_guard<std::mutex> lk(dedup_mu_);
    if (!dedup_table_) {
      // lazy init at default capacity
      uint64_t cap = 1ull << 22;
      dedup_table_ = DeviceBuffer(cap * 48);
      HIP_CHECK(hipMemsetAsync(dedup_table_.get(), 0, cap * 48, hash_stream_));
      dedup_cap_ = cap;
      dedup_dropped_ = DeviceBuffer(sizeof(uint32_t));
      HIP_CHECK(hipMemsetAsync(dedup_dropped_.get(), 0, sizeof(uint32_t), hash_stream_));
    }
    // one upload: n leaves (32 B each), then their n chunk indexes
    char* dleaves = ds_leaves_.reserve<char>(uniq.size());
    HIP_CHECK(hipMemcpyAsync(dleaves, uniq.data(), uniq.size(), hipMemcpyHostToDevice,
                             hash_stream_));
    const uint32_t* didx = reinterpret_cast<const uint32_t*>(dleaves + (size_t)n * 32);
    HIP_CHECK(modelx_dedup_insert(dleaves, didx, n, base, chunk_size, total,
                                  dedup_table_.get(), dedup_cap_,
                                  dedup_dropped_.get<uint32_t>(), hash_stream_));
    uint32_t dropped = 0;
    HIP_CHECK(hipStreamSynchronize(hash_stream_));
    HIP_CHECK(hipMemcpy(&dropped, dedup_dropped_.get(), sizeof dropped, hipMemcpyDeviceToHost));
    return dropped;
  }

  // Probe + gather resident chunks for an expected-leaves array; returns
  // (missing (offset,length) ranges merged, deduped_bytes).
  py::tuple dedup_pull(py::bytes expect, uintptr_t dst_ptr, uint64_t chunk_size,
                       uint64_t total) {
    std::string lv = expect;
    // the gather kernel writes chunk i at dst_ptr + i * chunk_size: a leaf
    // past the blob's end would be a write past the destination
    uint32_t n = checked_leaf_count("dedup_pull", lv.size(), chunk_size, total);
    std::vector<std::pair<uint64_t, uint64_t>> missing;
    uint64_t deduped = 0;
    if (total && dedup_table_) {
      HIP_CHECK(hipSetDevice(device_));
      py::gil_scoped_release release;
      std::lock_guard<std::mutex> lk(dedup_mu_);
      void* dleaves = ds_leaves_.reserve(lv.size());
      uint64_t* daddr = ds_addr_.reserve<uint64_t>((uint64_t)n * 8);
      uint64_t* dlen = ds_len_.reserve<uint64_t>((uint64_t)n * 8);
      HIP_CHECK(hipMemcpyAsync(dleaves, lv.data(), lv.size(), hipMemcpyHostToDevice,
                               hash_stream_));
      HIP_CHECK(modelx_dedup_probe(dleaves, n, chunk_size, total, dedup_table_.get(),
                                   dedup_cap_, daddr, dlen, hash_stream_));
      HIP_CHECK(modelx_dedup_gather(daddr, dlen, n, dst_ptr, chunk_size, hash_stream_));
      std::vector<uint64_t> haddr(n);
      HIP_CHECK(hipStreamSynchronize(hash_stream_));
      HIP_CHECK(hipMemcpy(haddr.data(), daddr, (uint64_t)n * 8, hipMemcpyDeviceToHost));
      for (uint32_t i = 0; i < n; i++) {
        uint64_t off = (uint64_t)i * chunk_size;
        uint64_t ln = total - off < chunk_size ? total - off : chunk_size;
        if (haddr[i] != 0) {
          deduped += ln;
        } else if (!missing.empty() && missing.back().first + missing.back().second == off) {
          missing.back().second += ln;
        } else {
          missing.emplace_back(off, ln);
        }
      }
    } else {
      if (total) missing.emplace_back(0, total);
    }
    py::list out;
    for (auto& m : missing) out.append(py::make_tuple(m.first, m.second));
    return py::make_tuple(out, deduped);
  }

  void synchronize() {
    HIP_CHECK(hipSetDevice(device_));
    for (auto& st : streams_) HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipStreamSynchronize(hash_stream_));
  }

 private:
  Slot* acquire_slot() {
    std::unique_lock<std::mutex> lk(mu_);
    cv_free_.wait(lk, [&] { return !free_.empty(); });
    Slot* s = free_.front();
    free_.pop();
    return s;
  }
  void release_slot(Slot* s) {
    {
      std::lock_guard<std::mutex> lk(mu_);
      free_.push(s);
    }
    cv_free_.notify_all();
  }

  // The two pinned slots of a double-buffered D2H drain. Both are taken in
  // ONE wait: sequential acquire_slot() would hold-and-wait and can deadlock
  // when >= num_slots drains run concurrently. The destructor waits out any
  // copy still in flight into a slot before the pool can hand it out again.
  class SlotLease {
   public:
    explicit SlotLease(GpuEngine& eng) : eng_(eng) {
      std::unique_lock<std::mutex> lk(eng_.mu_);
      eng_.cv_free_.wait(lk, [&] { return eng_.free_.size() >= 2; });
      for (Slot*& s : slot_) {
        s = eng_.free_.front();
        eng_.free_.pop();
      }
    }
    SlotLease(const SlotLease&) = delete;
    ~SlotLease() {
      for (int i = 0; i < 2; i++)
        if (in_flight_[i]) (void)hipEventSynchronize(slot_[i]->event);
      {
        std::lock_guard<std::mutex> lk(eng_.mu_);
        for (Slot* s : slot_) eng_.free_.push(s);
      }
      eng_.cv_free_.notify_all();
    }
    const char* host(int i) const { return slot_[i]->host; }
    // async D2H into slot i on st, then record the slot's event
    hipError_t fill(int i, const char* src, uint64_t len, hipStream_t st) {
      hipError_t e = hipMemcpyAsync(slot_[i]->host, src, len, hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipEventRecord(slot_[i]->event, st);
      if (e == hipSuccess) in_flight_[i] = true;
      return e;
    }
    hipError_t wait(int i) {
      in_flight_[i] = false;
      return hipEventSynchronize(slot_[i]->event);
    }

   private:
    GpuEngine& eng_;
    Slot* slot_[2];
    bool in_flight_[2] = {false, false};
  };

  // Stream [src_ptr, src_ptr+size) D2H through two leased pinned slots and
  // hand each filled (host_ptr, len) to `consume` in order, the copy into
  // one slot overlapping the consumer's work on the other. `consume`
  // returning false stops the drain; a HIP error stops it and is returned.
  template <class Consume>
  hipError_t drain_device(uintptr_t src_ptr, uint64_t size, Consume&& consume) {
    if (!size) return hipSuccess;
    const char* src = reinterpret_cast<const char*>(src_ptr);
    // streams chosen round-robin so concurrent drains (part uploads, blob
    // digests) don't serialize on one stream
    hipStream_t st_a = streams_[push_rr_.fetch_add(1) % streams_.size()];
    hipStream_t st_b = streams_[push_rr_.fetch_add(1) % streams_.size()];
    SlotLease lease(*this);
    int cur = 0, nxt = 1;
    uint64_t off = 0;
    uint64_t cur_len = std::min<uint64_t>(slot_bytes_, size);
    hipError_t e = lease.fill(cur, src, cur_len, st_a);
    while (e == hipSuccess && off < size) {
      uint64_t next_off = off + cur_len;
      uint64_t next_len = next_off < size ? std::min<uint64_t>(slot_bytes_, size - next_off) : 0;
      if (next_len) {
        e = lease.fill(nxt, src + next_off, next_len, st_b);
        if (e != hipSuccess) break;
        std::swap(st_a, st_b);
      }
      e = lease.wait(cur);
      if (e != hipSuccess || !consume(lease.host(cur), cur_len)) break;
      std::swap(cur, nxt);
      off = next_off;
      cur_len = next_len;
    }
    return e;
  }

  // start a ranged GET and validate the response head; body is then read
  // with read_body_exact by the caller. STRICT framing: must answer 206
  // with Content-Length == the requested span — a 200 (full object) or a
  // mismatched length would land the wrong bytes silently.
  bool begin_range_fetch(http::ClientConn& conn, const http::Url& u, http::Headers h,
                         const Range& r) {
    h["Range"] =
        "bytes=" + std::to_string(r.offset) + "-" + std::to_string(r.offset + r.length - 1);
    if (!conn.send_request("GET", u.target(), h, -1)) return false;
    int status = 0;
    http::Headers rh;
    if (!conn.read_response_head(&status, &rh)) return false;
    auto cl = rh.find("Content-Length");
    if (status != 206 || cl == rh.end() ||
        atoll(cl->second.c_str()) != static_cast<long long>(r.length)) {
      conn.close_fd();
      return false;
    }
    return true;
  }

  int device_;
  size_t slot_bytes_;
  std::atomic<int> push_rr_{0};
  std::vector<Slot> slots_;
  std::queue<Slot*> free_;
  std::deque<Slot*> pending_;
  std::vector<hipStream_t> streams_;
  hipStream_t hash_stream_ = nullptr;
  std::mutex mu_;
  std::condition_variable cv_free_, cv_pending_;
  ConnPool conn_pool_;
  // Everything below zstd_mu_ up to dedup_mu_ is guarded by zstd_mu_;
  // everything below dedup_mu_ by dedup_mu_. A scratch buffer is only valid
  // while its mutex is held: the next holder may reallocate it.
  std::mutex zstd_mu_;
  DeviceScratch zs_compress_, zs_seqs_, zs_sizes_, zs_segs_;  // zstd_compress_device
  // decode, single-blob and batched alike (rc: one entry per launched frame)
  DeviceScratch zs_frames_, zs_lit_, zs_rc_;
  hipEvent_t zs_staged_ = nullptr;  // frame array staged -> decode streams may start
  DeviceScratch zs_leaves_, zs_descs_;  // sha256_chunk_leaves_many
  std::mutex dedup_mu_;
  DeviceBuffer dedup_table_;
  uint64_t dedup_cap_ = 0;
  DeviceBuffer dedup_dropped_;  // one uint32_t
  DeviceScratch ds_leaves_, ds_addr_, ds_len_;
};

bool hip_available() {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess && n > 0;
}

int hip_device_count() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

}  // namespace

PYBIND11_MODULE(_core, m) {
  m.doc() = "modelx_amd native core: pinned-ring S3<->HBM engine + CDNA4 SHA-256 kernels";
  m.def("hip_available", &hip_available);
  m.def("hip_device_count", &hip_device_count);
  // PCI BDF of a device ("0000:0c:00.0") — lets callers find the GPU's
  // NUMA node via /sys/bus/pci/devices/<bdf>/numa_node and pin their
  // engine/server threads to it (measured +4-8% on the loopback bench)
  m.def("hip_pci_bus_id", [](int device) {
    char buf[64] = {};
    if (hipDeviceGetPCIBusId(buf, sizeof buf, device) != hipSuccess)
      throw std::runtime_error("hipDeviceGetPCIBusId failed");
    return std::string(buf);
  });

  py::class_<GpuEngine>(m, "GpuEngine")
      .def(py::init<int, int, size_t, int>(), py::arg("device") = 0, py::arg("num_slots") = 8,
           py::arg("slot_bytes") = (size_t)(64 << 20), py::arg("num_streams") = 4)
      .def("pull_to_device", &GpuEngine::pull_to_device, py::arg("url"), py::arg("headers"),
           py::arg("size"), py::arg("dst_ptr"), py::arg("num_conns") = 8,
           py::arg("base_offset") = 0)
      .def("pull_ranges_to_device", &GpuEngine::pull_ranges_to_device, py::arg("url"),
           py::arg("headers"), py::arg("ranges"), py::arg("dst_ptr"), py::arg("num_conns") = 8)
      .def("pull_to_device_hashed", &GpuEngine::pull_to_device_hashed, py::arg("url"),
           py::arg("headers"), py::arg("size"), py::arg("dst_ptr"), py::arg("num_conns") = 8,
           py::arg("chunk_size") = (uint64_t)(128 << 10))
      .def("sha256_chunk_leaves", &GpuEngine::sha256_chunk_leaves, py::arg("dev_ptr"),
           py::arg("size"), py::arg("chunk_size"))
      .def("sha256_multibuf", &GpuEngine::sha256_multibuf, py::arg("buffers"))
      .def("sha256_canonical_device", &GpuEngine::sha256_canonical_device,
           py::arg("src_ptr"), py::arg("size"))
      .def("read_device", &GpuEngine::read_device, py::arg("src_ptr"), py::arg("size"))
      .def("push_part_from_device", &GpuEngine::push_part_from_device, py::arg("url"),
           py::arg("method"), py::arg("headers"), py::arg("src_ptr"), py::arg("size"))
      .def("tar_index", &GpuEngine::tar_index, py::arg("tar_ptr"), py::arg("tar_len"))
      .def("tar_scatter", &GpuEngine::tar_scatter, py::arg("tar_ptr"), py::arg("segs"))
      .def("tar_pack", &GpuEngine::tar_pack, py::arg("dst_ptr"), py::arg("dst_cap"),
           py::arg("members"))
      .def("dedup_reset", &GpuEngine::dedup_reset, py::arg("cap_pow2") = (uint64_t)0)
      .def("dedup_register", &GpuEngine::dedup_register, py::arg("leaves"), py::arg("base"),
           py::arg("chunk_size"), py::arg("total"))
      .def("dedup_pull", &GpuEngine::dedup_pull, py::arg("expect"), py::arg("dst_ptr"),
           py::arg("chunk_size"), py::arg("total"))
      .def("zstd_decompress_many", &GpuEngine::zstd_decompress_many, py::arg("items"))
      .def("sha256_chunk_leaves_many", &GpuEngine::sha256_chunk_leaves_many,
           py::arg("items"))
      .def("zstd_compress_device", &GpuEngine::zstd_compress_device, py::arg("src_ptr"),
           py::arg("size"), py::arg("frame_raw"), py::arg("dst_ptr"), py::arg("dst_cap"),
           py::arg("literals_only") = false)
      .def("byte_planes", &GpuEngine::byte_planes, py::arg("items"), py::arg("merge"))
      .def("zstd_decompress_device", &GpuEngine::zstd_decompress_device, py::arg("src_ptr"),
           py::arg("src_len"), py::arg("dst_ptr"), py::arg("dst_cap"))
      .def("synchronize", &GpuEngine::synchronize);

  // Tar layout for an ordered [(name, size)] member list (tar_host.hpp):
  // header bytes, per-member offsets and the archive length. No GPU needed;
  // GpuEngine::tar_pack writes exactly this archive.
  m.def(
      "tar_pack_layout",
      [](const std::vector<std::pair<std::string, uint64_t>>& members) {
        tarhost::PackLayout lay = tarhost::pack_layout(members);
        py::list entries;
        for (auto& e : lay.entries) {
          py::dict d;
          d["header_off"] = e.header_off;
          d["header_len"] = e.header_len;
          d["payload_off"] = e.payload_off;
          d["size"] = e.size;
          entries.append(std::move(d));
        }
        py::dict out;
        out["headers"] = py::bytes(lay.headers);
        out["entries"] = entries;
        out["total"] = lay.total;
        return out;
      },
      py::arg("members"));
  // GpuEngine::tar_index on host bytes (tar_host.hpp): the same header walk
  // and name resolution, the same result and the same RuntimeErrors. No GPU
  // needed; the model the engine's index is tested against.
  m.def(
      "tar_index_host",
      [](py::bytes data) {
        std::string s = data;
        std::vector<tarhost::IndexedFile> files;
        {
          py::gil_scoped_release release;
          files = tarhost::index_host(reinterpret_cast<const uint8_t*>(s.data()), s.size());
        }
        return indexed_files_to_py(files);
      },
      py::arg("data"));
  m.def("zstd_compress_bound", &GpuEngine::zstd_compress_bound, py::arg("size"),
        py::arg("frame_raw") = (uint32_t)(128 << 10));
  // CPU codec path (same header-only core as the kernels) — used by the
  // CPU client for +zstd blobs and by tests as the GPU-vs-CPU oracle.
  m.def(
      "zstd_compress_cpu",
      [](py::bytes data, uint32_t frame_raw, bool literals_only) {
        std::string s = data;
        std::vector<uint8_t> out;
        {
          py::gil_scoped_release release;
          out = zstdhost::compress_seekable(reinterpret_cast<const uint8_t*>(s.data()),
                                            s.size(), frame_raw,
                                            literals_only ? zstd::kEncLiteralsOnly : 0u);
        }
        return py::bytes(reinterpret_cast<const char*>(out.data()), out.size());
      },
      py::arg("data"), py::arg("frame_raw") = (uint32_t)(128 << 10),
      py::arg("literals_only") = false);
  // The byte-plane transform's host model (byteplane_host.hpp): split
  // (merge=False) or merge of `data` at element size `elem` and group size
  // `group`. The CPU client's codec filter and the GPU kernels' oracle.
  m.def(
      "byte_planes_cpu",
      [](py::bytes data, uint64_t elem, uint64_t group, bool merge) {
        byteplane::validate(elem, group);
        std::string s = data;
        std::string out(s.size(), '\0');
        {
          py::gil_scoped_release release;
          const uint8_t* src = reinterpret_cast<const uint8_t*>(s.data());
          uint8_t* dst = reinterpret_cast<uint8_t*>(&out[0]);
          if (merge) byteplane::merge(src, dst, s.size(), static_cast<uint32_t>(elem), group);
          else byteplane::split(src, dst, s.size(), static_cast<uint32_t>(elem), group);
        }
        return py::bytes(out);
      },
      py::arg("data"), py::arg("elem"), py::arg("group"), py::arg("merge") = false);
  // One-shot GET through the NATIVE http client (the exact code path the
  // engine's ranged fetches use, incl. TLS) — lets the GPU-less suite prove
  // https presigned-URL support against a TLS server.
  m.def("http_get", [](const std::string& url,
                       const std::map<std::string, std::string>& headers) {
    http::Url u = http::Url::parse(url);
    http::ClientConn conn(u.host, u.port, u.scheme == "https");
    http::Headers h;
    for (auto& kv : headers) h[kv.first] = kv.second;
    h["Host"] = u.host + ":" + std::to_string(u.port);
    http::ClientResponse resp;
    if (!conn.do_request("GET", u.target(), h, "", &resp))
      throw std::runtime_error("http_get: request failed (connect/TLS/socket)");
    return py::make_tuple(resp.status, py::bytes(resp.body));
  }, py::arg("url"), py::arg("headers") = std::map<std::string, std::string>{});

  // CPU-testable canonical sha256 over host bytes — same OpenSSL EVP code
  // the D2H canonical path runs (lets the GPU-less suite oracle it against
  // hashlib)
  m.def("sha256_host", [](py::bytes data) {
    std::string s = data;
    unsigned char md[32];
    unsigned int mdlen = 0;
    EVP_MD_CTX* ctx = EVP_MD_CTX_new();
    if (!ctx || EVP_DigestInit_ex(ctx, EVP_sha256(), nullptr) != 1) {
      if (ctx) EVP_MD_CTX_free(ctx);
      throw std::runtime_error("EVP sha256 init failed");
    }
    EVP_DigestUpdate(ctx, s.data(), s.size());
    EVP_DigestFinal_ex(ctx, md, &mdlen);
    EVP_MD_CTX_free(ctx);
    return py::bytes(reinterpret_cast<char*>(md), 32);
  });
  m.def("zstd_decompress_cpu", [](py::bytes data) {
    std::string s = data;
    std::vector<uint8_t> out;
    {
      py::gil_scoped_release release;
      out = zstdhost::decompress(reinterpret_cast<const uint8_t*>(s.data()), s.size());
    }
    return py::bytes(reinterpret_cast<const char*>(out.data()), out.size());
  });
  m.def("zstd_content_size", [](py::bytes data) {
    std::string s = data;
    return zstdhost::content_size(reinterpret_cast<const uint8_t*>(s.data()), s.size());
  });
  auto entry_tuples = [](const std::vector<SeekEntry>& t) {
    py::list out;
    for (auto& e : t) out.append(py::make_tuple(e.c_off, e.c_size, e.d_off, e.d_size));
    return out;
  };
  m.def("zstd_frames", [=](py::bytes data) {
    std::string s = data;
    auto t = zstdhost::parse_seek_table(reinterpret_cast<const uint8_t*>(s.data()), s.size());
    if (t.empty())
      t = zstdhost::walk_frames(reinterpret_cast<const uint8_t*>(s.data()), s.size());
    return entry_tuples(t);
  });
  // The strict two-step seek-table parser the device decode paths rely on:
  // raises instead of falling back, so the GPU-less suite can test it.
  m.def("zstd_seek_table", [=](py::bytes data) {
    std::string s = data;
    const uint8_t* blob = reinterpret_cast<const uint8_t*>(s.data());
    uint8_t foot[zstdhost::kSeekFooterBytes] = {};
    if (s.size() >= sizeof foot) memcpy(foot, blob + s.size() - sizeof foot, sizeof foot);
    zstdhost::SeekFooter ft = zstdhost::parse_seek_footer(foot, s.size());
    std::vector<SeekEntry> t;
    zstdhost::parse_seek_entries(blob + s.size() - ft.table_bytes, ft, s.size(), &t);
    return entry_tuples(t);
  });
}
