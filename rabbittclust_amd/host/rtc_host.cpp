// rtc_host.cpp -- host side of the drop-in (see rtc_host.h).  Plain C++17 + zlib; no GPU code.
#include "rtc_host.h"
#include "../csrc/rtc_tree_medoid.h"

#include <ctype.h>
#include <dlfcn.h>
#include <errno.h>
#include <fcntl.h>
#include <unistd.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <time.h>
#include <atomic>
#include <cmath>
#include <zlib.h>
#if defined(__x86_64__)
#include <immintrin.h>  // the AVX2 / AVX-512 tiers of the FASTA intake; other hosts build the portable tier only
#define RTC_HOST_X86 1
#else
#define RTC_HOST_X86 0
#endif

#include <algorithm>
#include <unordered_map>
#include <type_traits>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <limits>
#include <queue>
#include <thread>

namespace rtc {

// =================================================================================================
// FASTA / FASTQ reader.  Behaviour follows klib kseq as the reference drives it
// (src/kseq.h:176-226 kseq_read, :92-140 ks_getuntil2):
//   * records start at a line whose first character is '>' or '@';
//   * name = header text up to the first isspace() character; comment = rest of the header line
//     (absent when the name is terminated by the newline);
//   * sequence = following lines concatenated, up to a line starting with '>', '@' or '+';
//     a trailing '\r' is dropped after each appended line when the accumulated length is > 1;
//   * '+' starts a FASTQ quality block: rest of that line skipped, then quality lines until the
//     quality is as long as the sequence.
// =================================================================================================
namespace {

// Byte source: zlib for gzip files; plain files (no 1f 8b magic) are read with read(2) directly,
// which yields the same bytes zlib's transparent mode would.
// gzip files of ordinary size are inflated in ONE call per member by libdeflate when the host has it (resolved with dlopen,
// no build dependency; about twice zlib's rate on sequence text), from a copy of the whole file in memory; the bytes are
// what gzread yields.  Anything it does not take -- no library, a file of more than 64 MiB, damaged or trailing data --
// goes through zlib's streaming gzread as before (which also defines what a damaged file yields).  RTC_NO_LIBDEFLATE=1: zlib only.
struct Deflate {
  void* (*alloc)() = nullptr;
  int (*gunzip_ex)(void*, const void*, size_t, void*, size_t, size_t*, size_t*) = nullptr;
  void (*release)(void*) = nullptr;
  static const Deflate& get() {
    static const Deflate d = []() {
      Deflate r;
      if (getenv("RTC_NO_LIBDEFLATE")) return r;
      void* h = dlopen("libdeflate.so.0", RTLD_NOW | RTLD_LOCAL);
      if (!h) h = dlopen("libdeflate.so", RTLD_NOW | RTLD_LOCAL);
      if (!h) return r;
      r.alloc = (void* (*)())dlsym(h, "libdeflate_alloc_decompressor");
      r.gunzip_ex = (int (*)(void*, const void*, size_t, void*, size_t, size_t*, size_t*))dlsym(h, "libdeflate_gzip_decompress_ex");
      r.release = (void (*)(void*))dlsym(h, "libdeflate_free_decompressor");
      if (!r.alloc || !r.gunzip_ex || !r.release) r = Deflate();
      return r;
    }();
    return d;
  }
};

class GzStream {
 public:
  explicit GzStream(const std::string& path) {
    fd_ = open(path.c_str(), O_RDONLY);
    if (fd_ < 0) return;
    unsigned char magic[2] = {0, 0};
    const ssize_t got = pread(fd_, magic, 2, 0);
    if (got == 2 && magic[0] == 0x1f && magic[1] == 0x8b) {
      if (!inflate_whole()) {
        f_ = gzdopen(fd_, "r");
        if (!f_) { close(fd_); fd_ = -1; return; }
        gzbuffer(f_, 1 << 20);
      }
    }
    buf_ = (char*)malloc(BUF + SLACK);
  }
  ~GzStream() {
    if (f_) gzclose(f_);  // closes fd_ too
    else if (fd_ >= 0) close(fd_);
    free(buf_);
    free(mem_);
  }
  GzStream(const GzStream&) = delete;
  GzStream& operator=(const GzStream&) = delete;
  bool ok() const { return fd_ >= 0 && buf_; }
  int getc() {
    if (begin_ >= end_) { if (!fill()) return -1; }
    return (unsigned char)buf_[begin_++];
  }
  // appends to `s` up to (not including) the delimiter class; returns the delimiter char or -1 at EOF.
  // mode 0: isspace()  mode 2: '\n'.  *gotany reports whether the stream had any data left.
  template <typename Sink>
  int get_until(int mode, Sink& s, bool append, bool* gotany) {
    if (!append) s.clear();
    *gotany = false;
    int dret = -1;
    for (;;) {
      if (begin_ >= end_) { if (!fill()) break; }
      int i = begin_;
      if (mode == 2) { const void* p = memchr(buf_ + begin_, '\n', end_ - begin_); i = p ? (int)((const char*)p - buf_) : end_; }
      else { for (; i < end_; ++i) if (isspace((unsigned char)buf_[i])) break; }
      *gotany = true;
      s.append(buf_ + begin_, i - begin_);
      begin_ = i + 1;
      if (i < end_) { dret = (unsigned char)buf_[i]; break; }
    }
    if (mode == 2 && s.size() > 1 && s.back() == '\r') s.pop_back();
    return dret;
  }
  bool eof() const { return eof_ && begin_ >= end_; }
  // Sequence-body fast path (the packed staging of the command lines, PackedSink::take_lines): hands the sink the buffer
  // from a line start on; the sink consumes the blocks that are plain sequence text and says whether it stopped inside a
  // line.  The general code continues from there -- finishing that line first -- and sees exactly the stream kseq's loop
  // would see at this point (src/SketchInfo.cpp:880-948 drives that loop).
  template <typename Sink>
  bool body_lines(Sink& s) {
    bool mid = false;
    if (begin_ < end_) begin_ += (int)s.take_lines(buf_ + begin_, (size_t)(end_ - begin_), &mid);
    return mid;
  }
  static constexpr int SLACK = 128;  // bytes a sink may read beyond the data it is handed (inside the allocation)
  // what decompression cost, summed over the parser threads (rtc_host_inflate_stats: the command lines' metrics)
  static std::atomic<uint64_t>& inflate_ns() { static std::atomic<uint64_t> v{0}; return v; }
  static std::atomic<uint64_t>& inflate_bytes() { static std::atomic<uint64_t> v{0}; return v; }
  static uint64_t now_ns() { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec; }

 private:
  static constexpr int BUF = 1 << 18;
  // the whole gzip file inflated into mem_ (every member in turn); false: leave it to zlib
  bool inflate_whole() {
    const Deflate& lib = Deflate::get();
    if (!lib.alloc) return false;
    struct stat st;
    if (fstat(fd_, &st) != 0 || st.st_size < 18 || st.st_size > ((off_t)64 << 20)) return false;  // (each parser thread holds one file inflated)
    const size_t csize = (size_t)st.st_size;
    unsigned char* comp = (unsigned char*)malloc(csize);
    if (!comp) return false;
    size_t have = 0;
    while (have < csize) {
      const ssize_t r = pread(fd_, comp + have, csize - have, (off_t)have);
      if (r < 0 && errno == EINTR) continue;
      if (r <= 0) break;
      have += (size_t)r;
    }
    bool ok = have == csize;
    void* d = ok ? lib.alloc() : nullptr;
    ok = ok && d;
    // One inflated file per parser thread: bounded at 1 GiB and at 64 x the compressed size (sequence text deflates
    // 3-4 x; a file that wants more -- crafted, or mostly one letter -- goes through zlib's streaming gzread, which
    // needs 1 MiB).  The trailing ISIZE (the last member's length mod 2^32) is only a first guess inside that bound.
    const size_t cap_max = std::min<size_t>((size_t)1 << 30, csize * 64 + 65536);
    uint32_t isize;
    memcpy(&isize, comp + csize - 4, 4);
    size_t cap = std::min(cap_max, std::max<size_t>((size_t)isize + 64, csize * 3)), out = 0, in = 0;
    char* mem = ok ? (char*)malloc(cap) : nullptr;
    ok = ok && mem;
    while (ok && in < csize) {
      if (csize - in < 18 || comp[in] != 0x1f || comp[in + 1] != 0x8b) { ok = false; break; }  // trailing bytes that are no member
      size_t used = 0, made = 0;
      const uint64_t t_in = now_ns();
      const int rc = lib.gunzip_ex(d, comp + in, csize - in, mem + out, cap - out, &used, &made);
      inflate_ns() += now_ns() - t_in;
      if (rc == 0) inflate_bytes() += made;
      if (rc == 3) {  // LIBDEFLATE_INSUFFICIENT_SPACE
        if (cap >= cap_max) { ok = false; break; }
        const size_t grown = std::min(cap_max, cap * 2);
        char* bigger = (char*)realloc(mem, grown);
        if (!bigger) { ok = false; break; }
        mem = bigger; cap = grown;
        continue;
      }
      if (rc != 0 || used == 0) { ok = false; break; }
      in += used; out += made;
    }
    if (d) lib.release(d);
    free(comp);
    if (!ok) { free(mem); return false; }
    mem_ = mem; mem_size_ = out; mem_pos_ = 0;
    return true;
  }
  bool fill() {
    if (eof_) return false;
    begin_ = 0;
    if (mem_) {
      const size_t n = std::min<size_t>((size_t)BUF, mem_size_ - mem_pos_);
      memcpy(buf_, mem_ + mem_pos_, n);
      mem_pos_ += n;
      end_ = (int)n;
    } else if (f_) {
      const uint64_t t_in = now_ns();  // (f_ is only ever a gzip stream)
      end_ = gzread(f_, buf_, BUF);
      if (end_ > 0) { inflate_ns() += now_ns() - t_in; inflate_bytes() += (uint64_t)end_; }
    }
    else {
      ssize_t r;
      do { r = read(fd_, buf_, BUF); } while (r < 0 && errno == EINTR);
      end_ = (int)r;
    }
    if (end_ <= 0) { end_ = 0; eof_ = true; return false; }
    return true;
  }
  int fd_ = -1;
  gzFile f_ = nullptr;
  char* mem_ = nullptr;            // a gzip file inflated whole (libdeflate), served through buf_ like the other sources
  size_t mem_size_ = 0, mem_pos_ = 0;
  char* buf_ = nullptr;
  int begin_ = 0, end_ = 0;
  bool eof_ = false;
};

// Sequence sink over a caller-supplied flat buffer.  size()/back()/pop_back() are relative to the
// current record, as kseq's seq.l is.  Writes beyond `cap` are dropped but still counted, so the
// caller learns the capacity a retry needs.
struct FlatSink {
  char* base; size_t cap;
  size_t pos = 0, rec = 0;
  void clear() { rec = pos; }
  void append(const char* p, size_t n) {
    if (pos + n <= cap) memcpy(base + pos, p, n);
    else if (pos < cap) memcpy(base + pos, p, cap - pos);
    pos += n;
  }
  void push_back(char c) { if (pos < cap) base[pos] = c; pos++; }
  size_t size() const { return pos - rec; }
  char back() const { return pos - 1 < cap ? base[pos - 1] : 0; }
  void pop_back() { pos--; }
};

// ---- 2-bit packed sink (the command lines' staging format: a quarter of the bytes over PCIe) ----
// Base i of the slot sits at bits 2 (i & 3) of byte i >> 2 with A, C, G, T (either case) = 0, 1, 2, 3.  Every other
// character -- N, IUPAC codes, the '\n' the reader puts between records -- is written as 0 and listed in `runs` as
// (start, length) in slot coordinates (ascending, adjacent ones merged): rtc_unpack_bases_dev turns the packed
// stream back into the ASCII the sketch kernels read and writes 'N' over the runs, which is all the kernels need
// (any character outside ACGT ends a k-mer the same way).  size()/back()/pop_back() behave as FlatSink's.
static inline uint32_t base_code(unsigned char c) { return ((c >> 1) ^ (c >> 2)) & 3u; }
static inline bool base_valid(unsigned char c) { return ((c & 0xC0u) == 0x40u) && ((0x0010008Au >> (c & 31u)) & 1u); }

struct PackedSink {
  uint8_t* base; size_t cap;           // cap in BASES
  std::vector<uint64_t>* runs;
  size_t pos = 0, rec = 0;             // bases appended so far / where the current record began
  // Lines are copied into a small character buffer first and packed a few KiB at a time: the packing loop then
  // always works on whole 32-base groups, whatever the line length of the file (60, 70, 80 ...).
  static constexpr size_t CH = 8192;
  size_t done = 0, fill = 0;           // stream positions [0, done) are packed, [done, done + fill) wait in buf
  unsigned char buf[CH + 32];  // (+ 32: headroom for the move of the unpacked remainder)
  PackedSink(uint8_t* b, size_t c, std::vector<uint64_t>* r) : base(b), cap(c), runs(r) {}
  void clear() { rec = pos; }
  size_t size() const { return pos - rec; }
  char back() const { return fill ? (char)buf[fill - 1] : 0; }
  void put1(unsigned char c) {         // packs one character at stream position `done`
    if (done < cap) {
      const uint32_t sh = 2 * (done & 3);
      const uint8_t code = base_valid(c) ? (uint8_t)(base_code(c) << sh) : 0;
      if (sh == 0) base[done >> 2] = code; else base[done >> 2] |= code;
      if (!base_valid(c)) {
        if (!runs->empty() && (*runs)[runs->size() - 2] + (*runs)[runs->size() - 1] == done) (*runs)[runs->size() - 1]++;
        else { runs->push_back(done); runs->push_back(1); }
      }
    }
    done++;
  }
  void emit(const unsigned char* p, size_t n);   // packs n characters at stream position `done`
  void flush(bool all) {
    const size_t m = all ? fill : fill & ~(size_t)31;
    emit(buf, m);
    const size_t rest = fill - m;  // < 32 unless everything went out
    for (size_t q = 0; q < rest; q++) buf[q] = buf[m + q];
    fill = rest;
  }
  void append(const char* p, size_t n) {
    while (n) {
      if (fill == CH) flush(false);
      const size_t k = n < CH - fill ? n : CH - fill;
      memcpy(buf + fill, p, k);
      fill += k; pos += k; p += k; n -= k;
    }
  }
  void push_back(char c) { append(&c, 1); }
#if RTC_HOST_X86
  // GzStream::body_lines: p is at a line start of a sequence body with `avail` valid bytes (and GzStream::SLACK readable
  // ones behind them).  Takes 32-byte blocks for as long as they hold nothing but sequence characters and '\n' -- no
  // '>', '@', '+' (a record start when first on a line) and no '\r' -- dropping the '\n's on the way: a block without one is
  // stored as it is, otherwise the pieces between the '\n's are stored one behind the other (each as a 32-byte store that the
  // next one overwrites from its own start; the buffer has the headroom).  No load depends on where the previous line
  // ended.  Returns the bytes consumed; *midline says whether they end inside a line, which the caller then finishes
  // with the general code (as it does everything from the first block that is not plain).
  __attribute__((target("avx2"))) size_t take_lines_avx2(const char* p, size_t avail, bool* midline) {
    const char* const p0 = p;
    const char* const e = p + avail;
    const __m256i nl = _mm256_set1_epi8('\n'), c1 = _mm256_set1_epi8('>'), c2 = _mm256_set1_epi8('@'), c3 = _mm256_set1_epi8('+'),
                  c4 = _mm256_set1_epi8('\r');
    bool mid = false;
    while (e - p >= 32) {
      const __m256i v = _mm256_loadu_si256((const __m256i*)p);
      const __m256i sp = _mm256_or_si256(_mm256_or_si256(_mm256_cmpeq_epi8(v, c1), _mm256_cmpeq_epi8(v, c2)),
                                         _mm256_or_si256(_mm256_cmpeq_epi8(v, c3), _mm256_cmpeq_epi8(v, c4)));
      if (_mm256_movemask_epi8(sp)) break;
      uint32_t m = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(v, nl));
      if (fill + 64 > CH) flush(false);  // leaves fill < 32
      unsigned char* d = buf + fill;
      if (!m) {
        _mm256_storeu_si256((__m256i*)d, v);
        fill += 32; pos += 32; mid = true;
      } else {
        uint32_t off = 0;
        do {
          const uint32_t k = (uint32_t)__builtin_ctz(m);
          _mm256_storeu_si256((__m256i*)d, _mm256_loadu_si256((const __m256i*)(p + off)));
          d += k - off; off = k + 1; m &= m - 1;
        } while (m);
        _mm256_storeu_si256((__m256i*)d, _mm256_loadu_si256((const __m256i*)(p + off)));
        d += 32 - off;
        const size_t got = (size_t)(d - (buf + fill));
        fill += got; pos += got; mid = off < 32;
      }
      p += 32;
    }
    *midline = mid;
    return (size_t)(p - p0);
  }
  // the same with 64-byte blocks: the four comparisons write mask registers, and ONE vpcompressb drops the '\n's
  __attribute__((target("avx512f,avx512bw,avx512vbmi2"))) size_t take_lines_avx512(const char* p, size_t avail, bool* midline) {
    const char* const p0 = p;
    const char* const e = p + avail;
    const __m512i nl = _mm512_set1_epi8('\n'), c1 = _mm512_set1_epi8('>'), c2 = _mm512_set1_epi8('@'), c3 = _mm512_set1_epi8('+'),
                  c4 = _mm512_set1_epi8('\r');
    bool mid = false;
    while (e - p >= 64) {
      const __m512i v = _mm512_loadu_si512((const void*)p);
      if (_mm512_cmpeq_epi8_mask(v, c1) | _mm512_cmpeq_epi8_mask(v, c2) | _mm512_cmpeq_epi8_mask(v, c3) | _mm512_cmpeq_epi8_mask(v, c4)) break;
      const __mmask64 m = _mm512_cmpeq_epi8_mask(v, nl);
      if (fill + 64 > CH) flush(false);  // leaves fill < 32; the buffer has room for one whole block behind CH - 32
      _mm512_storeu_si512((void*)(buf + fill), _mm512_maskz_compress_epi8(~m, v));
      const size_t got = 64 - (size_t)__builtin_popcountll(m);
      fill += got; pos += got;
      mid = !(m >> 63);
      p += 64;
    }
    *midline = mid;
    return (size_t)(p - p0);
  }
#endif
  size_t take_lines(const char* p, size_t avail, bool* midline);
  void truncate(size_t p) {  // drop everything from base p on (pop_back of a '\r', a record cut short)
    pos = p;
    if (p >= done) { fill = p - done; return; }
    fill = 0; done = p;
    if (p < cap && (p & 3)) base[p >> 2] &= (uint8_t)((1u << (2 * (p & 3))) - 1u);
    while (!runs->empty()) {
      uint64_t& st = (*runs)[runs->size() - 2]; uint64_t& ln = (*runs)[runs->size() - 1];
      if (st >= p) { runs->pop_back(); runs->pop_back(); }
      else { if (st + ln > p) ln = p - st; break; }
    }
  }
  void pop_back() { truncate(pos - 1); }
  void finish() { flush(true); }
};

#if RTC_HOST_X86
// 32 bases at a time: codes by two shifts and a mask, validity by re-encoding the codes (pshufb) and comparing with
// the upper-cased input, packing by two multiply-adds (c0 + 4 c1, then + 16 * (c2 + 4 c3)) and a byte gather
__attribute__((target("avx2"))) static size_t pack_run_avx2(const unsigned char* p, size_t n, uint8_t* out) {
  const __m256i m3 = _mm256_set1_epi8(3), mdf = _mm256_set1_epi8((char)0xDF);
  const __m256i lut = _mm256_setr_epi8('A', 'C', 'G', 'T', 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 'A', 'C', 'G', 'T', 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0);
  const __m256i w1 = _mm256_set1_epi16(0x0401), w2 = _mm256_set1_epi32(0x00100001);
  const __m256i gather = _mm256_setr_epi8(0, 4, 8, 12, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 4, 8, 12, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1);
  size_t i = 0;
  for (; i + 32 <= n; i += 32) {
    const __m256i x = _mm256_loadu_si256((const __m256i*)(p + i));
    const __m256i c = _mm256_and_si256(_mm256_xor_si256(_mm256_srli_epi16(x, 1), _mm256_srli_epi16(x, 2)), m3);
    const __m256i ok = _mm256_cmpeq_epi8(_mm256_shuffle_epi8(lut, c), _mm256_and_si256(x, mdf));
    if ((uint32_t)_mm256_movemask_epi8(ok) != 0xffffffffu) break;  // a character outside ACGTacgt: the caller goes base by base
    const __m256i q = _mm256_shuffle_epi8(_mm256_madd_epi16(_mm256_maddubs_epi16(c, w1), w2), gather);
    const uint32_t lo = (uint32_t)_mm256_cvtsi256_si32(q), hi = (uint32_t)_mm256_extract_epi32(q, 4);
    memcpy(out + (i >> 2), &lo, 4);
    memcpy(out + (i >> 2) + 4, &hi, 4);
  }
  return i;
}

// the same 64 bases at a time: validity as one 64-bit mask, the 16 packed bytes out of the 16 dwords by one down-convert
__attribute__((target("avx512f,avx512bw"))) static size_t pack_run_avx512(const unsigned char* p, size_t n, uint8_t* out) {
  const __m512i m3 = _mm512_set1_epi8(3), mdf = _mm512_set1_epi8((char)0xDF);
  const __m512i lut = _mm512_broadcast_i32x4(_mm_setr_epi8('A', 'C', 'G', 'T', 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0));
  const __m512i w1 = _mm512_set1_epi16(0x0401), w2 = _mm512_set1_epi32(0x00100001);
  size_t i = 0;
  for (; i + 64 <= n; i += 64) {
    const __m512i x = _mm512_loadu_si512((const void*)(p + i));
    const __m512i c = _mm512_and_si512(_mm512_xor_si512(_mm512_srli_epi16(x, 1), _mm512_srli_epi16(x, 2)), m3);
    if (_mm512_cmpeq_epi8_mask(_mm512_shuffle_epi8(lut, c), _mm512_and_si512(x, mdf)) != ~(__mmask64)0) break;
    const __m512i q = _mm512_madd_epi16(_mm512_maddubs_epi16(c, w1), w2);
    _mm_storeu_si128((__m128i*)(out + (i >> 2)), _mm512_cvtepi32_epi8(q));
  }
  return i;
}

#endif

// portable form of the same, 8 bases at a time in a 64-bit word
static size_t pack_run_swar(const unsigned char* p, size_t n, uint8_t* out) {
  size_t i = 0;
  for (; i + 8 <= n; i += 8) {
    uint64_t x;
    memcpy(&x, p + i, 8);
    const uint64_t c = ((x >> 1) ^ (x >> 2)) & 0x0303030303030303ULL;
    const uint64_t b0 = c & 0x0101010101010101ULL, b1 = (c >> 1) & 0x0101010101010101ULL;
    const uint64_t e = 0x4141414141414141ULL + 2 * b0 + 6 * b1 + 0x0B * (b0 & b1);   // A, C, G, T from the codes
    if ((x & 0xDFDFDFDFDFDFDFDFULL) != e) break;
    uint64_t t = (c | (c >> 6)) & 0x000F000F000F000FULL;
    t = (t | (t >> 12)) & 0x000000FF000000FFULL;
    t = t | (t >> 24);
    out[i >> 2] = (uint8_t)t; out[(i >> 2) + 1] = (uint8_t)(t >> 8);
  }
  return i;
}

// SIMD tier of the packer and of the line intake: 0 = the best the CPU has (AVX-512 BW + VBMI2, else AVX2, else portable),
// 1 = portable only, 2 = at most AVX2 (tests run every tier)
static int g_pack_portable = 0;
static int simd_tier() {  // 3: AVX-512, 2: AVX2, 1: portable
#if !RTC_HOST_X86
  return 1;
#else
  static const bool a512 = __builtin_cpu_supports("avx512f") && __builtin_cpu_supports("avx512bw") && __builtin_cpu_supports("avx512vbmi2");
  static const bool a2 = __builtin_cpu_supports("avx2");
  if (g_pack_portable == 1) return 1;
  if (a512 && g_pack_portable != 2) return 3;
  return a2 ? 2 : 1;
#endif
}
size_t PackedSink::take_lines(const char* p, size_t avail, bool* midline) {
  *midline = false;
  const int tier = simd_tier();
  size_t k = 0;
#if RTC_HOST_X86
  if (tier == 3) k = take_lines_avx512(p, avail, midline);
  if (tier >= 2 && avail - k >= 32) {
    // (what the 64-byte blocks left: a block with a special character in it, or fewer than 64 bytes) -- the 32-byte blocks get
    // as far as they can; they start where the wider ones stopped, inside a line or not
    bool mid2 = false;
    const size_t k2 = take_lines_avx2(p + k, avail - k, &mid2);
    if (k2) *midline = mid2;
    k += k2;
  }
#else
  (void)tier; (void)p; (void)avail;
#endif
  return k;
}

void PackedSink::emit(const unsigned char* p, size_t n) {
  const int tier = simd_tier();
  size_t i = 0;
  while (i < n) {
    if ((done & 3) == 0 && done + (n - i) <= cap && n - i >= 8) {  // byte-aligned, room for all: whole groups at once
      size_t k = 0;
#if RTC_HOST_X86
      if (tier == 3) k = pack_run_avx512(p + i, n - i, base + (done >> 2));   // 64 at a time, then the rest of the run below
      if (tier >= 2) k += pack_run_avx2(p + i + k, n - i - k, base + ((done + k) >> 2));
      else
#endif
        k = pack_run_swar(p + i, n - i, base + (done >> 2));
      done += k; i += k;
      if (i >= n) break;
    }
    // up to the next group boundary (or past the character the fast loop stopped at) one by one
    size_t k = 0;
    do { put1(p[i++]); k++; } while (i < n && ((done & 3) != 0 || k < 8));
  }
}

// returns sequence length, -1 at EOF, -2 on truncated quality
template <typename Sink>
int next_record_t(GzStream& ks, int& last_char, std::string& name, std::string& comment, bool& has_comment, Sink& seq) {
  int c;
  if (last_char == 0) {
    while ((c = ks.getc()) != -1 && c != '>' && c != '@') {}
    if (c == -1) return -1;
    last_char = c;
  }
  comment.clear(); seq.clear(); has_comment = false;
  bool got;
  int d = ks.get_until(0, name, false, &got);
  if (!got && ks.eof()) return -1;
  if (d != '\n' && d != -1) { ks.get_until(2, comment, false, &got); has_comment = true; }
  for (;;) {
    if constexpr (std::is_same<Sink, PackedSink>::value) {  // plain sequence text inside the buffer, 32 bytes at a time
      if (ks.body_lines(seq)) { ks.get_until(2, seq, true, &got); continue; }  // it stopped inside a line: the rest of that line
    }
    if ((c = ks.getc()) == -1 || c == '>' || c == '+' || c == '@') break;
    if (c == '\n') continue;
    seq.push_back((char)c);
    ks.get_until(2, seq, true, &got);
  }
  if (c == '>' || c == '@') last_char = c;
  if (c != '+') return (int)seq.size();
  while ((c = ks.getc()) != -1 && c != '\n') {}
  if (c == -1) return -2;
  std::string qual;
  while (true) {
    ks.get_until(2, qual, true, &got);
    if ((!got && ks.eof()) || qual.size() >= seq.size()) break;
  }
  last_char = 0;
  if (qual.size() != seq.size()) return -2;
  return (int)seq.size();
}

int next_record(GzStream& ks, int& last_char, FastaRecord& r) {
  return next_record_t(ks, last_char, r.name, r.comment, r.has_comment, r.seq);
}

}  // namespace
void rtc_host_inflate_stats(double* seconds, uint64_t* bytes_out) {
  if (seconds) *seconds = (double)GzStream::inflate_ns().load() * 1e-9;
  if (bytes_out) *bytes_out = GzStream::inflate_bytes().load();
}

bool read_fasta(const std::string& path, std::vector<FastaRecord>& out) {
  GzStream ks(path);
  if (!ks.ok()) return false;
  int last_char = 0;
  FastaRecord r;
  while (next_record(ks, last_char, r) >= 0) out.push_back(r);
  return true;
}

bool read_genome_file(const std::string& path, std::string& bases, SequenceInfo& first, uint64_t& total_len,
                      uint64_t& n_records) {
  GzStream ks(path);
  if (!ks.ok()) return false;
  int last_char = 0;
  FastaRecord r;
  total_len = 0; n_records = 0;
  int len;
  while ((len = next_record(ks, last_char, r)) >= 0) {
    total_len += (uint64_t)len;                                       // src/SketchInfo.cpp:933
    if (n_records == 0) {                                             // :934-947, only the first record is kept
      first.name = r.name;
      first.comment = r.has_comment ? r.comment : std::string("noName");
      first.strand = 0;
      first.length = len;
    }
    bases.append(r.seq);
    bases.push_back('\n');  // record separator: any non-ACGT byte resets the k-mer window
    n_records++;
  }
  return true;
}

uint64_t genome_slot_bytes(const std::string& path) {
  struct stat st;
  if (stat(path.c_str(), &st) != 0) return 0;
  uint64_t sz = (uint64_t)st.st_size;
  FILE* fp = fopen(path.c_str(), "rb");
  if (!fp) return 0;
  unsigned char magic[2] = {0, 0};
  const bool gz = fread(magic, 1, 2, fp) == 2 && magic[0] == 0x1f && magic[1] == 0x8b;
  if (gz && sz >= 18) {
    uint32_t isize = 0;
    fseek(fp, -4, SEEK_END);
    if (fread(&isize, 4, 1, fp) != 1) isize = 0;
    sz = std::max<uint64_t>(isize, sz);  // single-member guess; the reader reports the exact need on overflow
  }
  fclose(fp);
  return sz + 1;
}

int read_genome_file_flat(const std::string& path, char* dst, uint64_t cap, uint64_t& used, SequenceInfo& first,
                          uint64_t& total_len, uint64_t& n_records) {
  GzStream ks(path);
  if (!ks.ok()) return 1;
  int last_char = 0;
  std::string name, comment;
  bool has_comment = false;
  FlatSink sink{dst, (size_t)cap};
  total_len = 0; n_records = 0;
  int len;
  while ((len = next_record_t(ks, last_char, name, comment, has_comment, sink)) >= 0) {
    total_len += (uint64_t)len;
    if (n_records == 0) {
      first.name = name;
      first.comment = has_comment ? comment : std::string("noName");
      first.strand = 0;
      first.length = len;
    }
    sink.push_back('\n');
    n_records++;
  }
  // a record that ends on a truncated quality block (-2) stops the reader like kseq_read() < 0 does;
  // bases appended for it are not part of any returned record
  if (len == -2) sink.pos = sink.rec;
  used = sink.pos;
  return sink.pos > cap ? 2 : 0;
}

int read_genome_file_packed(const std::string& path, uint8_t* dst, uint64_t cap_bases, uint64_t& used, std::vector<uint64_t>& runs,
                            SequenceInfo& first, uint64_t& total_len, uint64_t& n_records) {
  GzStream ks(path);
  if (!ks.ok()) return 1;
  int last_char = 0;
  std::string name, comment;
  bool has_comment = false;
  runs.clear();
  PackedSink sink(dst, (size_t)cap_bases, &runs);
  total_len = 0; n_records = 0;
  int len;
  while ((len = next_record_t(ks, last_char, name, comment, has_comment, sink)) >= 0) {
    total_len += (uint64_t)len;
    if (n_records == 0) {
      first.name = name;
      first.comment = has_comment ? comment : std::string("noName");
      first.strand = 0;
      first.length = len;
    }
    sink.push_back('\n');
    n_records++;
  }
  if (len == -2) { const size_t want = sink.pos; sink.truncate(sink.rec); if (want > cap_bases) { used = want; return 2; } }
  sink.finish();
  used = sink.pos;
  return sink.pos > cap_bases ? 2 : 0;
}

void pack_force_portable(int on) { g_pack_portable = on; }

size_t pack_bases(const char* seq, size_t n, uint8_t* dst, std::vector<uint64_t>& runs) {
  runs.clear();
  PackedSink sink(dst, n, &runs);
  sink.append(seq, n);
  sink.finish();
  return sink.pos;
}

// =================================================================================================
// calSize (list mode), src/SketchInfo.cpp:438-482,536-552
// =================================================================================================
bool cal_size(const std::string& list_file, uint64_t minLen, uint64_t& maxSize, uint64_t& minSize, uint64_t& averageSize) {
  maxSize = 0; minSize = 1u << 31; averageSize = 0;
  uint64_t totalSize = 0; int number = 0, badNumber = 0;
  std::ifstream ifs(list_file);
  if (!ifs) { std::cerr << "ERROR: calSize(), cannot open the inputFile: " << list_file << std::endl; return false; }
  std::string line;
  while (getline(ifs, line)) {
    if (line.size() < 2) continue;
    uint64_t curSize;
    if (line.substr(line.length() - 2) == "gz") {
      FILE* fp = fopen(line.c_str(), "r");
      if (!fp) { std::cerr << "cannot open the genome file: " << line << std::endl; return false; }
      fseek(fp, -4, SEEK_END);
      int nUnCompress = 0;
      if (fread(&nUnCompress, sizeof(int), 1, fp) != 1) nUnCompress = 0;
      curSize = (uint64_t)(int64_t)nUnCompress;
      fclose(fp);
    } else {
      struct stat statbuf;
      if (stat(line.c_str(), &statbuf) != 0) { std::cerr << "cannot open the genome file: " << line << std::endl; return false; }
      curSize = (uint64_t)statbuf.st_size;
    }
    if (curSize < minLen) { badNumber++; continue; }
    maxSize = std::max(maxSize, curSize); minSize = std::min(minSize, curSize);
    totalSize += curSize; number++;
  }
  if (number == 0) { std::cerr << "ERROR: calSize(), no genome passes the minimum length filter" << std::endl; return false; }
  averageSize = totalSize / number;
  int totalNumber = number + badNumber;
  std::cerr << "\t===the genome number for clustering is: " << number << std::endl;
  std::cerr << "\t===the genome number below the minimum genome length threshold is: " << badNumber << std::endl;
  std::cerr << "\t===the total genome number is: " << totalNumber << std::endl;
  if ((double)badNumber / totalNumber >= 0.2)
    fprintf(stderr, "Warning: there are %d poor quality (length < %ld) genome assemblies in the total %d genome assemblied.\n",
            badNumber, (long)minLen, totalNumber);
  std::cerr << "\t===the totalSize is: " << totalSize << std::endl;
  std::cerr << "\t===the maxSize is: " << maxSize << std::endl;
  std::cerr << "\t===the minSize is: " << minSize << std::endl;
  std::cerr << "\t===the averageSize is: " << averageSize << std::endl;
  return true;
}

int file_length_for_containment(const std::string& path) {
  FILE* fp = fopen(path.c_str(), "r");
  if (!fp) return 0;
  int fileLength = 0;
  if (path.size() >= 2 && path.substr(path.length() - 2) == "gz") {
    fseek(fp, -4, SEEK_END);
    int nUnCompress = 0;
    if (fread(&nUnCompress, sizeof(int), 1, fp) != 1) nUnCompress = 0;
    fileLength = nUnCompress;
  } else {
    fseek(fp, 0, SEEK_END);
    fileLength = (int)ftell(fp);
  }
  fclose(fp);
  return fileLength;
}

// src/sub_command.cpp:2383-2467
bool tune_parameters(bool greedy, bool isSetKmer, uint64_t maxSize, uint64_t minSize, uint64_t averageSize,
                     bool& isContainment, bool isJaccard, int& kmerSize, double threshold, int& containCompress,
                     int sketchSize) {
  if (isContainment && isJaccard) {
    std::cerr << "ERROR: tune_parameters(), conflict distance measurement of Mash distance (fixed-sketch-size) and AAF distance (variable-sketch-size) " << std::endl;
    return false;
  }
  if (greedy) {
    if (!isContainment && !isJaccard) { containCompress = (int)(averageSize / 1000); isContainment = true; }
    else if (!isContainment && isJaccard) { }
    else if (averageSize / containCompress < 10) {
      std::cerr << "the containCompress " << containCompress << " is too large and the sketch size is too small" << std::endl;
      containCompress = (int)(averageSize / 1000);
      std::cerr << "set the containCompress to: " << containCompress << std::endl;
    }
  }
  double warning_rate = 0.01, recommend_rate = 0.0001;
  int recommendedKmerSize = (int)ceil(log(maxSize * (1 - recommend_rate) / recommend_rate) / log(4));
  int warningKmerSize = (int)ceil(log(maxSize * (1 - warning_rate) / warning_rate) / log(4));
  if (!isSetKmer) kmerSize = recommendedKmerSize;
  else if (kmerSize < warningKmerSize) {
    std::cerr << "the kmerSize " << kmerSize << " is too small for the maximum genome size of " << maxSize << std::endl;
    std::cerr << "replace the kmerSize to the: " << recommendedKmerSize << " for reducing the random collision of kmers" << std::endl;
    kmerSize = recommendedKmerSize;
  } else if (kmerSize > recommendedKmerSize + 3) {
    std::cerr << "the kmerSize " << kmerSize << " maybe too large for the maximum genome size of " << maxSize << std::endl;
    std::cerr << "replace the kmerSize to the " << recommendedKmerSize << " for increasing the sensitivity of genome comparison" << std::endl;
    kmerSize = recommendedKmerSize;
  }
  double minJaccard;
  if (!isContainment) minJaccard = 1.0 / sketchSize;
  else minJaccard = 1.0 / (minSize / containCompress);
  double maxDist = minJaccard >= 1.0 ? 1.0 : -1.0 / kmerSize * log(2 * minJaccard / (1.0 + minJaccard));
  std::cerr << "-----the max recommand distance threshold is: " << maxDist << std::endl;
  if (threshold > maxDist) {
    std::cerr << "ERROR: tune_parameters(), the threshold: " << threshold << " is out of the valid distance range estimated by Mash distance or AAF distance" << std::endl;
    std::cerr << "Please set a distance threshold with -d option" << std::endl;
    return false;
  }
  std::cerr << "-----the kmerSize is: " << kmerSize << std::endl;
  std::cerr << "-----the threshold is: " << threshold << std::endl;
  if (isContainment) std::cerr << "-----use the AAF distance (variable-sketch-size), the sketchSize is in proportion with 1/" << containCompress << std::endl;
  else std::cerr << "-----use the Mash distance (fixed-sketch-size), the sketchSize is: " << sketchSize << std::endl;
  return true;
}

// src/sub_command.cpp:2317-2381
bool tune_kssd_parameters(bool isSetKmer, uint64_t maxSize, uint64_t minSize, uint64_t averageSize, bool isContainment,
                          int& kmerSize, double threshold, int drlevel) {
  int compression = 1 << (4 * drlevel);
  int sketchSize = (int)(averageSize / compression);
  double warning_rate = 0.01, recommend_rate = 0.0001;
  int recommendedKmerSize = (int)ceil(log(maxSize * (1 - recommend_rate) / recommend_rate) / log(4));
  int warningKmerSize = (int)ceil(log(maxSize * (1 - warning_rate) / warning_rate) / log(4));
  if (!isSetKmer) kmerSize = recommendedKmerSize;
  else if (kmerSize < warningKmerSize) {
    std::cerr << "the kmerSize " << kmerSize << " is too small for the maximum genome size of " << maxSize << std::endl;
    std::cerr << "replace the kmerSize to the: " << recommendedKmerSize << " for reducing the random collision of kmers" << std::endl;
    kmerSize = recommendedKmerSize;
  } else if (kmerSize > recommendedKmerSize + 3) {
    std::cerr << "the kmerSize " << kmerSize << " maybe too large for the maximum genome size of " << maxSize << std::endl;
    std::cerr << "replace the kmerSize to the " << recommendedKmerSize << " for increasing the sensitivity of genome comparison" << std::endl;
    kmerSize = recommendedKmerSize;
  }
  double minJaccard;
  if (!isContainment) minJaccard = 1.0 / sketchSize;
  else minJaccard = 1.0 / (minSize / compression);
  double maxDist = minJaccard >= 1.0 ? 1.0 : -1.0 / kmerSize * log(2 * minJaccard / (1.0 + minJaccard));
  std::cerr << "-----the max recommand distance threshold is: " << maxDist << std::endl;
  if (threshold > maxDist) {
    std::cerr << "ERROR: tune_parameters(), the threshold: " << threshold << " is out of the valid distance range estimated by Mash distance or AAF distance" << std::endl;
    std::cerr << "Please set a distance threshold with -d option" << std::endl;
    return false;
  }
  std::cerr << "-----the kmerSize is: " << kmerSize << std::endl;
  std::cerr << "-----the threshold is: " << threshold << std::endl;
  return true;
}

// src/SketchInfo.cpp:60-102: two Fisher-Yates passes driven by glibc srand()/rand().
// The generator is restated here (glibc random_r TYPE_3: 31-word additive feedback r[i] = r[i-3] +
// r[i-31], seeded by the Lehmer recurrence 16807*x mod 2^31-1, first 310 outputs discarded, result
// >> 1) so the table does not depend on the C library in use and the draws can be produced a block
// ahead of the swaps, which lets the swap targets be prefetched.  tests/test_cpu_host.py pins the
// table against the golden one made with the C library's own rand().
namespace {
struct GlibcRand {
  int32_t r[34];
  int f, b;  // front / rear indices into the 31-word state
  explicit GlibcRand(unsigned seed) {
    int32_t st[31];
    st[0] = seed ? (int32_t)seed : 1;
    for (int i = 1; i < 31; i++) {
      const long hi = st[i - 1] / 127773, lo = st[i - 1] % 127773;
      long word = 16807 * lo - 2836 * hi;
      if (word < 0) word += 2147483647;
      st[i] = (int32_t)word;
    }
    for (int i = 0; i < 31; i++) r[i] = st[i];
    f = 3; b = 0;
    for (int i = 0; i < 310; i++) next();
  }
  inline int32_t next() {
    const uint32_t v = (uint32_t)r[f] + (uint32_t)r[b];
    r[f] = (int32_t)v;
    if (++f == 31) f = 0;
    if (++b == 31) b = 0;
    return (int32_t)(v >> 1);
  }
};
}  // namespace

std::vector<int32_t> generate_shuffle_dim(int half_subk) {
  const int dim_size = 1 << (4 * half_subk);
  std::vector<int32_t> arr(dim_size);
  for (int i = 0; i < dim_size; i++) arr[i] = i;
  const unsigned seeds[2] = {23u, 348842630u};
  constexpr int BLK = 64;
  int js[2][BLK];
  for (unsigned seed : seeds) {
    GlibcRand g(seed);
    // draws for block `nb` are made (and their targets prefetched) while block `nb-1` is swapped
    auto draw = [&](int* out, int i_hi, int cnt) {
      for (int q = 0; q < cnt; q++) { out[q] = g.next() % (i_hi - q + 1); __builtin_prefetch(&arr[out[q]], 1); }
    };
    int i = dim_size - 1, cur = 0;
    int cnt = std::min(BLK, i);
    draw(js[cur], i, cnt);
    while (cnt > 0) {
      const int i_next = i - cnt;
      const int cnt_next = std::min(BLK, i_next);
      if (cnt_next > 0) draw(js[cur ^ 1], i_next, cnt_next);
      for (int q = 0; q < cnt; q++) std::swap(arr[i - q], arr[js[cur][q]]);
      i = i_next; cnt = cnt_next; cur ^= 1;
    }
  }
  return arr;
}

// =================================================================================================
// on-disk formats
// =================================================================================================
namespace {
template <typename T> void wr(FILE* fp, const T& v) { fwrite(&v, sizeof(T), 1, fp); }
template <typename T> bool rd(FILE* fp, T& v) { return fread(&v, sizeof(T), 1, fp) == 1; }
FILE* open_or_die(const std::string& path, const char* mode, const char* who) {
  FILE* fp = fopen(path.c_str(), mode);
  if (!fp) { std::cerr << "ERROR: " << who << ", cannot open the file: " << path << std::endl; exit(1); }
  return fp;
}
}  // namespace

// src/Sketch_IO.cpp:36-134: info.sketch / info.mst / kssd.info.sketch / kssd.info.mst
void save_genome_info(const std::vector<GenomeInfo>& g, const std::string& folder, const std::string& type,
                      bool sketchByFile, bool kssd) {
  const std::string path = folder + '/' + (kssd ? "kssd.info." : "info.") + type;
  FILE* fp = open_or_die(path, "w+", "save_genome_info()");
  wr(fp, sketchByFile);
  size_t n = g.size();
  wr(fp, n);
  for (const GenomeInfo& s : g) {
    if (sketchByFile) {
      int a = (int)s.fileName.length(), b = (int)s.seq0.name.length(), c = (int)s.seq0.comment.length();
      wr(fp, a); wr(fp, b); wr(fp, c); wr(fp, s.seq0.strand); wr(fp, s.totalSeqLength);
      fwrite(s.fileName.c_str(), 1, a, fp); fwrite(s.seq0.name.c_str(), 1, b, fp); fwrite(s.seq0.comment.c_str(), 1, c, fp);
    } else {
      int b = (int)s.seq0.name.length(), c = (int)s.seq0.comment.length();
      wr(fp, b); wr(fp, c); wr(fp, s.seq0.strand); wr(fp, s.seq0.length);
      fwrite(s.seq0.name.c_str(), 1, b, fp); fwrite(s.seq0.comment.c_str(), 1, c, fp);
    }
    if (kssd) wr(fp, s.use64);
  }
  fclose(fp);
}

bool load_genome_info(const std::string& folder, const std::string& type, std::vector<GenomeInfo>& g, bool kssd,
                      bool& sketchByFile) {
  const std::string path = folder + '/' + (kssd ? "kssd.info." : "info.") + type;
  FILE* fp = fopen(path.c_str(), "r");
  if (!fp) { std::cerr << "ERROR: load_genome_info(), cannot open file: " << path << std::endl; return false; }
  size_t n = 0;
  if (!rd(fp, sketchByFile) || !rd(fp, n)) { fclose(fp); return false; }
  g.clear(); g.reserve(n);
  auto rdstr = [&](int len, std::string& s) { s.resize(len > 0 ? len : 0); return len <= 0 || fread(&s[0], 1, len, fp) == (size_t)len; };
  for (size_t i = 0; i < n; i++) {
    GenomeInfo s; s.id = (int)i;
    if (sketchByFile) {
      int a, b, c;
      if (!rd(fp, a) || !rd(fp, b) || !rd(fp, c) || !rd(fp, s.seq0.strand) || !rd(fp, s.totalSeqLength)) { fclose(fp); return false; }
      if (!rdstr(a, s.fileName) || !rdstr(b, s.seq0.name) || !rdstr(c, s.seq0.comment)) { fclose(fp); return false; }
    } else {
      int b, c;
      if (!rd(fp, b) || !rd(fp, c) || !rd(fp, s.seq0.strand) || !rd(fp, s.seq0.length)) { fclose(fp); return false; }
      if (!rdstr(b, s.seq0.name) || !rdstr(c, s.seq0.comment)) { fclose(fp); return false; }
    }
    if (kssd && !rd(fp, s.use64)) { fclose(fp); return false; }
    g.push_back(std::move(s));
  }
  fclose(fp);
  return true;
}

// src/Sketch_IO.cpp:169-226 (MinHash branch)
void save_minhash_sketches(const std::vector<GenomeInfo>& g, const MinHashSketchFile& f, const std::string& folder,
                           bool sketchByFile) {
  save_genome_info(g, folder, "sketch", sketchByFile, false);
  FILE* fp = open_or_die(folder + "/hash.sketch", "w+", "saveSketch()");
  int sketch_func_id = 0;
  wr(fp, sketch_func_id); wr(fp, f.kmerSize); wr(fp, f.isContainment);
  if (f.isContainment) wr(fp, f.containCompress); else wr(fp, f.sketchSize);
  for (const auto& h : f.hashes) { size_t m = h.size(); wr(fp, m); fwrite(h.data(), sizeof(uint64_t), m, fp); }
  fclose(fp);
  std::cerr << "-----save the sketches into: " << folder << std::endl;
}

// src/Sketch_IO.cpp:284-353
bool load_minhash_sketches(const std::string& folder, std::vector<GenomeInfo>& g, MinHashSketchFile& f, bool& sketchByFile) {
  FILE* fp = fopen((folder + "/hash.sketch").c_str(), "r");
  if (!fp) {
    std::cerr << "ERROR: loadSketches(), cannot open the file: " << folder << "/hash.sketch" << std::endl;
    FILE* t = fopen((folder + "/kssd.hash.sketch").c_str(), "r");
    if (t) { std::cerr << "Do you want to load the kssd sketches directory? Try again with '--fast' option" << std::endl; fclose(t); }
    return false;
  }
  int sketch_func_id = 0;
  if (!rd(fp, sketch_func_id) || sketch_func_id != 0) { fclose(fp); std::cerr << "ERROR: loadSketches(), only MinHash sketch folders are supported" << std::endl; return false; }
  if (!rd(fp, f.kmerSize) || !rd(fp, f.isContainment)) { fclose(fp); return false; }
  if (f.isContainment) { if (!rd(fp, f.containCompress)) { fclose(fp); return false; } }
  else if (!rd(fp, f.sketchSize)) { fclose(fp); return false; }
  if (!load_genome_info(folder, "sketch", g, false, sketchByFile)) { fclose(fp); return false; }
  f.hashes.assign(g.size(), {});
  for (size_t i = 0; i < g.size(); i++) {
    size_t m = 0;
    if (!rd(fp, m)) { fclose(fp); return false; }
    f.hashes[i].resize(m);
    if (m && fread(f.hashes[i].data(), sizeof(uint64_t), m, fp) != m) { fclose(fp); return false; }
  }
  fclose(fp);
  return true;
}

// src/SketchInfo.h:115-160 "MHIDX001".  Entries are written in ascending hash order (the reference
// writes hash-map iteration order; its loader accepts any order).
void save_minhash_index(const MinHashSketchFile& f, const std::string& folder) {
  std::vector<std::pair<uint64_t, uint32_t>> all;
  size_t tot = 0;
  for (const auto& h : f.hashes) tot += h.size();
  all.reserve(tot);
  for (size_t g = 0; g < f.hashes.size(); g++) for (uint64_t h : f.hashes[g]) all.emplace_back(h, (uint32_t)g);
  std::sort(all.begin(), all.end());
  size_t nuniq = 0;
  for (size_t i = 0; i < all.size(); i++) if (i == 0 || all[i].first != all[i - 1].first) nuniq++;
  FILE* fp = fopen((folder + "/minhash.sketch.index").c_str(), "wb");
  if (!fp) { std::cerr << "WARNING: cannot save MinHash index to: " << folder << "/minhash.sketch.index" << std::endl; return; }
  fwrite("MHIDX001", 1, 8, fp);
  wr(fp, nuniq);
  for (size_t i = 0; i < all.size();) {
    size_t j = i;
    while (j < all.size() && all[j].first == all[i].first) j++;
    uint64_t h = all[i].first; uint32_t m = (uint32_t)(j - i);
    wr(fp, h); wr(fp, m);
    for (size_t t = i; t < j; t++) wr(fp, all[t].second);
    i = j;
  }
  fclose(fp);
  std::cerr << "-----MinHash inverted index saved: " << folder << "/minhash.sketch.index (" << nuniq << " unique hashes)" << std::endl;
}

// src/Sketch_IO.cpp:136-167
void save_kssd_sketches(const std::vector<GenomeInfo>& g, const KssdSketchFile& f, const std::string& folder, bool sketchByFile) {
  save_genome_info(g, folder, "sketch", sketchByFile, true);
  FILE* fp = open_or_die(folder + "/kssd.hash.sketch", "w+", "saveSketch()");
  fwrite(&f.info, sizeof(KssdParameters), 1, fp);
  for (size_t i = 0; i < g.size(); i++) {
    if (f.use64) { size_t m = f.h64[i].size(); wr(fp, m); fwrite(f.h64[i].data(), sizeof(uint64_t), m, fp); }
    else { size_t m = f.h32[i].size(); wr(fp, m); fwrite(f.h32[i].data(), sizeof(uint32_t), m, fp); }
  }
  fclose(fp);
  std::cerr << "-----save the kssd sketches into: " << folder << std::endl;
}

// src/Sketch_IO.cpp:228-282
bool load_kssd_sketches(const std::string& folder, std::vector<GenomeInfo>& g, KssdSketchFile& f, bool& sketchByFile) {
  FILE* fp = fopen((folder + "/kssd.hash.sketch").c_str(), "r");
  if (!fp) {
    std::cerr << "ERROR: loadKssdSketches(), cannot open the file: " << folder << "/kssd.hash.sketch" << std::endl;
    FILE* t = fopen((folder + "/hash.sketch").c_str(), "r");
    if (t) { std::cerr << "Do you want to load the minHash sketches directory? Try again without '--fast' option" << std::endl; fclose(t); }
    return false;
  }
  if (fread(&f.info, sizeof(KssdParameters), 1, fp) != 1) { fclose(fp); return false; }
  if (!load_genome_info(folder, "sketch", g, true, sketchByFile) || g.empty()) { fclose(fp); return false; }
  f.use64 = g[0].use64;
  f.h32.assign(f.use64 ? 0 : g.size(), {}); f.h64.assign(f.use64 ? g.size() : 0, {});
  for (size_t i = 0; i < g.size(); i++) {
    size_t m = 0;
    if (!rd(fp, m)) { fclose(fp); return false; }
    if (f.use64) { f.h64[i].resize(m); if (m && fread(f.h64[i].data(), 8, m, fp) != m) { fclose(fp); return false; } }
    else { f.h32[i].resize(m); if (m && fread(f.h32[i].data(), 4, m, fp) != m) { fclose(fp); return false; } }
  }
  fclose(fp);
  return true;
}

// src/SketchInfo.cpp:1379-1467: kssd.sketch.index = {size_t H; hash[H]; u32 count[H]}, .dict = ids
void save_kssd_index(const KssdSketchFile& f, const std::string& folder) {
  std::vector<std::pair<uint64_t, uint32_t>> all;
  const size_t n = f.use64 ? f.h64.size() : f.h32.size();
  for (size_t g = 0; g < n; g++) {
    if (f.use64) for (uint64_t h : f.h64[g]) all.emplace_back(h, (uint32_t)g);
    else for (uint32_t h : f.h32[g]) all.emplace_back((uint64_t)h, (uint32_t)g);
  }
  std::sort(all.begin(), all.end());
  std::vector<uint64_t> keys; std::vector<uint32_t> counts;
  FILE* fd = open_or_die(folder + "/kssd.sketch.dict", "w+", "transSketchesFromIndex");
  for (size_t i = 0; i < all.size();) {
    size_t j = i;
    while (j < all.size() && all[j].first == all[i].first) j++;
    keys.push_back(all[i].first); counts.push_back((uint32_t)(j - i));
    for (size_t t = i; t < j; t++) wr(fd, all[t].second);
    i = j;
  }
  fclose(fd);
  FILE* fi = open_or_die(folder + "/kssd.sketch.index", "w+", "transSketchesFromIndex");
  size_t H = keys.size();
  wr(fi, H);
  if (f.use64) fwrite(keys.data(), 8, H, fi);
  else for (uint64_t k : keys) { uint32_t k32 = (uint32_t)k; wr(fi, k32); }
  fwrite(counts.data(), 4, H, fi);
  fclose(fi);
}

// src/MST_IO.cpp:200-217, :47-70
void save_mst(const std::vector<rtc_edge>& mst, const std::string& folder) {
  FILE* fp = open_or_die(folder + "/edge.mst", "w+", "saveMST()");
  size_t m = mst.size();
  wr(fp, m);
  for (const rtc_edge& e : mst) { wr(fp, e.preNode); wr(fp, e.sufNode); wr(fp, e.dist); }
  fclose(fp);
  std::cerr << "-----save the mst into: " << folder << std::endl;
}
bool load_mst(const std::string& folder, std::vector<rtc_edge>& mst) {
  FILE* fp = fopen((folder + "/edge.mst").c_str(), "r");
  if (!fp) { std::cerr << "ERROR: loadMST(), cannot open the file: " << folder << "/edge.mst" << std::endl; return false; }
  size_t m = 0;
  if (!rd(fp, m)) { fclose(fp); return false; }
  mst.clear(); mst.reserve(m);
  for (size_t i = 0; i < m; i++) {
    rtc_edge e;
    if (!rd(fp, e.preNode) || !rd(fp, e.sufNode) || !rd(fp, e.dist)) { fclose(fp); return false; }
    mst.push_back(e);
  }
  fclose(fp);
  std::cerr << "-----read the mst file from " << folder << "/edge.mst" << std::endl;
  return true;
}

// =================================================================================================
// forest cut + BFS clusters + text output
// =================================================================================================
void save_dense(const std::string& folder, const std::vector<int32_t>& dense, int span, int genome_number) {  // src/MST_IO.cpp:219-233
  const std::string file = folder + "/mst.dense";
  FILE* fp = fopen(file.c_str(), "w+");
  if (!fp) { std::cerr << "ERROR: saveDense(), cannot open the file: " << file; exit(1); }
  fwrite(&genome_number, sizeof(int), 1, fp);
  fwrite(&span, sizeof(int), 1, fp);
  fwrite(dense.data(), sizeof(int32_t), (size_t)span * genome_number, fp);
  fclose(fp);
  std::cerr << "-----save the dense file into: " << folder << std::endl;
}

bool load_dense(const std::string& folder, std::vector<int32_t>& dense, int& span, int& genome_number) {  // src/MST_IO.cpp:12-28
  const std::string file = folder + "/mst.dense";
  FILE* fp = fopen(file.c_str(), "r");
  if (!fp) { std::cerr << "ERROR: saveDense(), cannot open the file: " << file; return false; }
  bool ok = fread(&genome_number, sizeof(int), 1, fp) == 1 && fread(&span, sizeof(int), 1, fp) == 1 && span >= 0 && genome_number >= 0;
  if (ok) {
    dense.resize((size_t)span * genome_number);
    ok = fread(dense.data(), sizeof(int32_t), dense.size(), fp) == dense.size();
  }
  fclose(fp);
  if (ok) std::cerr << "-----read the dense file from: " << file << std::endl;
  return ok;
}

void save_ani(const std::string& folder, const uint64_t ani[101]) {  // src/MST_IO.cpp:235-250
  const std::string file = folder + "/mst.ani";
  FILE* fp = fopen(file.c_str(), "w+");
  if (!fp) { std::cerr << "ERROR: saveANI(), cannot open file: " << file << std::endl; exit(1); }
  fwrite(ani, sizeof(uint64_t), 101, fp);
  fclose(fp);
  std::cerr << "-----save the ani file into: " << file << std::endl;
}

bool load_ani(const std::string& folder, uint64_t ani[101]) {
  FILE* fp = fopen((folder + "/mst.ani").c_str(), "r");
  if (!fp) return false;
  const bool ok = fread(ani, sizeof(uint64_t), 101, fp) == 101;
  fclose(fp);
  return ok;
}

std::vector<int> noise_nodes(const std::vector<std::vector<int>>& cluster, const std::vector<int32_t>& dense, int span,
                             int genome_number, double threshold) {  // src/sub_command.cpp:3077-3092, src/MST.cpp:189-211
  const int alpha = 2;
  const int denseIndex = (int)(threshold / 0.01);
  std::vector<int> total;
  if (denseIndex < 0 || denseIndex >= span) return total;
  for (const std::vector<int>& cl : cluster) {
    if (cl.size() == 1) continue;
    std::vector<std::pair<int, int>> arr;
    for (int element : cl) arr.emplace_back(element, dense[(size_t)denseIndex * genome_number + element]);
    std::sort(arr.begin(), arr.end(), [](const std::pair<int, int>& a, const std::pair<int, int>& b) { return a.second < b.second; });  // cmpPair
    const int denseQ1 = arr[arr.size() / 4].second;
    int thr = std::max(std::min(denseQ1 - 1, alpha), 0);
    for (const auto& p : arr) { if (p.second <= thr) total.push_back(p.first); else break; }
  }
  return total;
}

std::vector<rtc_edge> modify_forest(const std::vector<rtc_edge>& forest, const std::vector<int>& noise) {  // src/MST.cpp:86-107
  std::vector<char> is_noise;
  for (int v : noise) { if ((size_t)v >= is_noise.size()) is_noise.resize(v + 1, 0); is_noise[v] = 1; }
  std::vector<rtc_edge> out;
  for (const rtc_edge& e : forest) {
    const bool rm = ((size_t)e.preNode < is_noise.size() && is_noise[e.preNode]) || ((size_t)e.sufNode < is_noise.size() && is_noise[e.sufNode]);
    if (!rm) out.push_back(e);
  }
  return out;
}

namespace {
struct DSU {  // src/MST.cpp:40-57
  std::vector<int> p, r;
  explicit DSU(int n) : p(n), r(n, 0) { for (int i = 0; i < n; i++) p[i] = i; }
  int find(int x) { int root = x; while (p[root] != root) root = p[root]; while (p[x] != root) { int nx = p[x]; p[x] = root; x = nx; } return root; }
  int unite(int a, int b) {
    a = find(a); b = find(b);
    if (a == b) return a;
    if (r[a] < r[b]) std::swap(a, b);
    p[b] = a;
    if (r[a] == r[b]) r[a]++;
    return a;
  }
};
std::vector<rtc_edge> by_distance(const std::vector<rtc_edge>& mst) {
  std::vector<rtc_edge> edges = mst;
  std::sort(edges.begin(), edges.end(), [](const rtc_edge& a, const rtc_edge& b) { return a.dist < b.dist; });
  return edges;
}
}  // namespace

// Newick text of the single-linkage dendrogram the MST defines (what src/MST.cpp:1044-1150 prints): edges in ascending
// weight (std::sort with the reference's comparator, so ties fall as they do there) merge the sets of their two ends; a
// merge is an inner node at height = the edge's weight whose first branch leads to the top node of preNode's set and
// whose second to sufNode's, branch length = height difference (never negative); the text starts at the top node of
// genome 0's set.  Merges live in one flat array (node id = leaves + merge number), the sets in a plain parent array
// with the set's current top node kept at its representative, and the text is written by an explicit stack (a
// caterpillar of 100 000 leaves would overflow a recursive writer).
std::string get_newick_tree(const std::vector<GenomeInfo>& g, const std::vector<rtc_edge>& mst, bool sketchByFile) {
  const int leaves = (int)g.size();
  auto label = [&](int v) -> const std::string& { return sketchByFile ? g[v].fileName : g[v].seq0.name; };
  if (leaves == 0) return ";";
  if (leaves == 1) return label(0) + ";";
  struct Merge { int kid[2]; double len[2]; double at; };
  std::vector<Merge> merges;
  merges.reserve(leaves - 1);
  std::vector<int> set_of(leaves), top(leaves);
  for (int v = 0; v < leaves; v++) set_of[v] = top[v] = v;
  auto rep = [&](int v) { while (set_of[v] != v) { set_of[v] = set_of[set_of[v]]; v = set_of[v]; } return v; };
  auto level = [&](int node) { return node < leaves ? 0.0 : merges[node - leaves].at; };
  for (const rtc_edge& e : by_distance(mst)) {
    const int a = rep(e.preNode), b = rep(e.sufNode);
    if (a == b) continue;
    Merge m;
    m.kid[0] = top[a]; m.kid[1] = top[b];
    m.at = e.dist;
    for (int side = 0; side < 2; side++) m.len[side] = std::max(0.0, m.at - level(m.kid[side]));
    merges.push_back(m);
    set_of[b] = a;
    top[a] = leaves + (int)merges.size() - 1;
  }
  std::string text;
  struct Visit { int node; int done; };  // done: how many of an inner node's two branches are written
  std::vector<Visit> path{{top[rep(0)], 0}};
  while (!path.empty()) {
    Visit& v = path.back();
    if (v.node < leaves) {
      text += label(v.node);
    } else if (v.done < 2) {
      text += v.done == 0 ? "(" : ",";
      const int kid = merges[v.node - leaves].kid[v.done++];
      path.push_back({kid, 0});
      continue;
    } else {
      text += ")";
    }
    path.pop_back();
    if (!path.empty()) {  // the subtree just closed hangs on branch done-1 of the node now on top
      const Visit& up = path.back();
      text += ":" + std::to_string(merges[up.node - leaves].len[up.done - 1]);
    }
  }
  return text + ";";
}

// Newick text of one neighbour-joining tree from its records (include/rtclust.h: rtc_njoin; a, b and c are genome indices).
// text(x) is the subtree currently named x: a leaf at first, after a join {a, b} the node "(text(a):len_a,text(b):len_b)" under
// the name a; the last record of three or more members has three children and closes the tree.  One member: "label;", two:
// "(a:x,b:y);".  The nodes live in one flat array and the text is written by an explicit stack, as get_newick_tree's.
//
// With support (rtc_nj_support's counts, one per record, of `replicates`): in a tree of four or more members every node of a
// record with c == UINT32_MAX names a split and carries nj_support_percent between its ")" and its ":"; the closing node and
// smaller trees carry nothing.  Without it the text is the plain one, and the labelled text with the labels taken out is too.
std::string nj_support_newick_text(const std::function<std::string(uint32_t)>& label, const uint32_t* members, size_t m, const rtc_njoin* joins,
                                   size_t n_joins, const uint32_t* support, uint32_t replicates) {
  if (m == 0) return ";";
  if (m == 1 || n_joins == 0) return label(members[0]) + ";";
  struct Node { int kid[3]; double len[3]; int nk; };
  std::vector<Node> nodes;
  nodes.reserve(n_joins);
  std::unordered_map<uint32_t, int> named;  // the node a name stands for: below m the leaf members[.], from m on nodes[. - m]
  named.reserve(2 * m);
  for (size_t v = 0; v < m; v++) named[members[v]] = (int)v;
  for (size_t e = 0; e < n_joins; e++) {
    const rtc_njoin& r = joins[e];
    Node nd;
    nd.nk = r.c == 0xFFFFFFFFu ? 2 : 3;
    const uint32_t name[3] = {r.a, r.b, r.c};
    const double len[3] = {r.len_a, r.len_b, r.len_c};
    for (int s = 0; s < 3; s++) { nd.kid[s] = s < nd.nk ? named.at(name[s]) : -1; nd.len[s] = len[s]; }
    nodes.push_back(nd);
    named[r.a] = (int)(m + nodes.size() - 1);
  }
  const int leaves = (int)m;
  std::string text;
  struct Visit { int node; int done; };  // done: how many of an inner node's branches are written
  std::vector<Visit> path{{leaves + (int)nodes.size() - 1, 0}};
  while (!path.empty()) {
    Visit& v = path.back();
    if (v.node < leaves) {
      text += label(members[v.node]);
    } else if (v.done < nodes[v.node - leaves].nk) {
      text += v.done == 0 ? "(" : ",";
      const int kid = nodes[v.node - leaves].kid[v.done++];
      path.push_back({kid, 0});
      continue;
    } else {
      text += ")";
      if (support && m >= 4 && nodes[v.node - leaves].nk == 2) text += std::to_string(nj_support_percent(support[v.node - leaves], replicates));
    }
    path.pop_back();
    if (!path.empty()) {  // the subtree just closed hangs on branch done-1 of the node now on top
      const Visit& up = path.back();
      text += ":" + std::to_string(nodes[up.node - leaves].len[up.done - 1]);
    }
  }
  return text + ";";
}

std::string nj_newick_text(const std::function<std::string(uint32_t)>& label, const uint32_t* members, size_t m, const rtc_njoin* joins,
                           size_t n_joins) {
  return nj_support_newick_text(label, members, m, joins, n_joins, nullptr, 0);
}

// The table of one tree's labelled nodes, a line a record that names a split, in record order:
// cluster \t record \t leaves below the node \t count \t replicates
std::string nj_support_tsv_lines(size_t cluster, size_t m, const rtc_njoin* joins, size_t n_joins, const uint32_t* support, uint32_t replicates) {
  std::string text;
  if (m < 4) return text;
  std::unordered_map<uint32_t, uint64_t> below;  // the leaves under the node a name stands for (a name not seen yet: one leaf)
  for (size_t e = 0; e < n_joins; e++) {
    const rtc_njoin& r = joins[e];
    if (r.c != 0xFFFFFFFFu) continue;
    auto leaves = [&](uint32_t x) { auto it = below.find(x); return it == below.end() ? (uint64_t)1 : it->second; };
    const uint64_t s = leaves(r.a) + leaves(r.b);
    below[r.a] = s;
    text += std::to_string(cluster) + "\t" + std::to_string(e) + "\t" + std::to_string(s) + "\t" + std::to_string(support[e]) + "\t" +
            std::to_string(replicates) + "\n";
  }
  return text;
}

std::string get_nj_newick(const std::vector<GenomeInfo>& g, const std::vector<int>& members, const rtc_njoin* joins, size_t n_joins,
                          bool sketchByFile) {
  std::vector<uint32_t> mem(members.begin(), members.end());
  std::sort(mem.begin(), mem.end());
  return nj_newick_text([&](uint32_t v) { return sketchByFile ? g[v].fileName : g[v].seq0.name; }, mem.data(), mem.size(), joins, n_joins);
}

static FILE* open_out(const std::string& output, const char* who) {
  FILE* fp = fopen(output.c_str(), "w");
  if (!fp) { std::cerr << "ERROR: " << who << "(), cannot write file: " << output << std::endl; exit(1); }
  return fp;
}

void print_newick_tree(const std::vector<GenomeInfo>& g, const std::vector<rtc_edge>& mst, bool sketchByFile, const std::string& output) {
  FILE* fp = open_out(output, "print_newick_tree");
  fprintf(fp, "%s\n", get_newick_tree(g, mst, sketchByFile).c_str());
  fclose(fp);
}

// One tree a line, one line a cluster, in the order of `clusters`; first[q] .. first[q + 1] are the records of the cluster whose
// smallest member is the q-th smallest (rtc_nj_clusters' component order).
void print_nj_newick(const std::vector<GenomeInfo>& g, const std::vector<std::vector<int>>& clusters, const std::vector<rtc_njoin>& joins,
                     const std::vector<uint64_t>& first, bool sketchByFile, const std::string& output) {
  std::vector<size_t> order(clusters.size()), rank(clusters.size());
  std::vector<int> smallest(clusters.size());
  for (size_t c = 0; c < clusters.size(); c++) { order[c] = c; smallest[c] = *std::min_element(clusters[c].begin(), clusters[c].end()); }
  std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return smallest[x] < smallest[y]; });
  for (size_t q = 0; q < order.size(); q++) rank[order[q]] = q;
  FILE* fp = open_out(output, "print_nj_newick");
  for (size_t c = 0; c < clusters.size(); c++) {
    const size_t q = rank[c];
    fprintf(fp, "%s\n", get_nj_newick(g, clusters[c], joins.data() + first[q], (size_t)(first[q + 1] - first[q]), sketchByFile).c_str());
  }
  fclose(fp);
}

// print_nj_newick's trees with their support (newick), and the counts (tsv): a header, then the lines of nj_support_tsv_lines tree
// after tree in the order of `clusters`, the cluster numbered as `clusters` lists it.
void print_nj_support(const std::vector<GenomeInfo>& g, const std::vector<std::vector<int>>& clusters, const std::vector<rtc_njoin>& joins,
                      const std::vector<uint64_t>& first, const std::vector<uint32_t>& support, uint32_t replicates, bool sketchByFile,
                      const std::string& newick, const std::string& tsv) {
  std::vector<size_t> order(clusters.size()), rank(clusters.size());
  std::vector<int> smallest(clusters.size());
  for (size_t c = 0; c < clusters.size(); c++) { order[c] = c; smallest[c] = *std::min_element(clusters[c].begin(), clusters[c].end()); }
  std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return smallest[x] < smallest[y]; });
  for (size_t q = 0; q < order.size(); q++) rank[order[q]] = q;
  FILE* fn = open_out(newick, "print_nj_support");
  FILE* ft = open_out(tsv, "print_nj_support");
  fprintf(ft, "cluster\trecord\tleaves\tcount\treplicates\n");
  for (size_t c = 0; c < clusters.size(); c++) {
    const size_t q = rank[c];
    const size_t nr = (size_t)(first[q + 1] - first[q]);
    std::vector<uint32_t> mem(clusters[c].begin(), clusters[c].end());
    std::sort(mem.begin(), mem.end());
    fprintf(fn, "%s\n", nj_support_newick_text([&](uint32_t v) { return sketchByFile ? g[v].fileName : g[v].seq0.name; }, mem.data(), mem.size(),
                                               joins.data() + first[q], nr, support.data() + first[q], replicates).c_str());
    fputs(nj_support_tsv_lines(c, mem.size(), joins.data() + first[q], nr, support.data() + first[q], replicates).c_str(), ft);
  }
  fclose(fn);
  fclose(ft);
}

bool upgma_keep(uint64_t sum, uint32_t size_a, uint32_t size_b, double threshold) {
  const long long qcut = llround(threshold * 1048576.0);
  if (qcut < 0) return false;
  return (unsigned __int128)sum <= (unsigned __int128)(uint64_t)qcut * ((uint64_t)size_a * (uint64_t)size_b);
}

uint64_t upgma_report(uint32_t n, const std::vector<std::vector<int>>& clusters, const rtc_umerge* merges, const uint64_t* first, double threshold,
                      std::string* linkage_txt, std::vector<std::vector<int>>* refined) {
  std::vector<size_t> order(clusters.size());
  std::vector<int> smallest(clusters.size());
  for (size_t c = 0; c < clusters.size(); c++) { order[c] = c; smallest[c] = *std::min_element(clusters[c].begin(), clusters[c].end()); }
  std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return smallest[x] < smallest[y]; });
  std::vector<int> cid(n), head(n);  // the linkage id of the cluster named g; the refined cluster (index into out) named g
  for (uint32_t g = 0; g < n; g++) cid[g] = (int)g;
  std::vector<std::vector<int>> out;
  int next_id = (int)n;
  uint64_t kept = 0;
  char buf[128];
  linkage_txt->clear();
  for (size_t q = 0; q < order.size(); q++) {
    const size_t out0 = out.size();
    for (int g : clusters[order[q]]) { head[g] = (int)out.size(); out.push_back({g}); }
    bool cut = false;
    for (uint64_t e = first[q]; e < first[q + 1]; e++) {
      const rtc_umerge& mg = merges[e];
      snprintf(buf, sizeof buf, "%d\t%d\t%.6f\t%u\n", cid[mg.a], cid[mg.b], upgma_height(mg.sum, mg.size_a, mg.size_b), mg.size_a + mg.size_b);
      *linkage_txt += buf;
      cid[mg.a] = next_id++;
      if (!cut && !upgma_keep(mg.sum, mg.size_a, mg.size_b, threshold)) cut = true;
      if (cut) continue;
      std::vector<int>& A = out[head[mg.a]];
      std::vector<int>& B = out[head[mg.b]];
      A.insert(A.end(), B.begin(), B.end());
      B.clear();
      kept++;
    }
    std::vector<std::vector<int>> part;
    for (size_t i = out0; i < out.size(); i++) if (!out[i].empty()) { std::sort(out[i].begin(), out[i].end()); part.push_back(std::move(out[i])); }
    out.resize(out0);
    for (auto& c : part) out.push_back(std::move(c));
  }
  std::sort(out.begin(), out.end(), [](const std::vector<int>& x, const std::vector<int>& y) { return x[0] < y[0]; });
  *refined = std::move(out);
  return kept;
}

// The records become binary rtc_njoin records -- len = the new node's height minus the child's -- and nj_newick_text writes them.
std::string upgma_newick_text(const std::function<std::string(uint32_t)>& label, const uint32_t* members, size_t m, const rtc_umerge* merges,
                              size_t n_merges) {
  std::unordered_map<uint32_t, double> height;  // of the cluster named g; a leaf is at 0
  height.reserve(2 * m);
  std::vector<rtc_njoin> joins(n_merges);
  for (size_t e = 0; e < n_merges; e++) {
    const rtc_umerge& mg = merges[e];
    const double h = upgma_height(mg.sum, mg.size_a, mg.size_b) / 2.0;
    const auto ia = height.find(mg.a), ib = height.find(mg.b);
    const double ha = ia == height.end() ? 0.0 : ia->second, hb = ib == height.end() ? 0.0 : ib->second;
    joins[e] = rtc_njoin{mg.a, mg.b, 0xFFFFFFFFu, 0u, h - ha, h - hb, 0.0};
    height[mg.a] = h;
  }
  return nj_newick_text(label, members, m, joins.data(), n_merges);
}

void print_upgma_newick(const std::vector<GenomeInfo>& g, const std::vector<std::vector<int>>& clusters, const std::vector<rtc_umerge>& merges,
                        const std::vector<uint64_t>& first, bool sketchByFile, const std::string& output) {
  std::vector<size_t> order(clusters.size()), rank(clusters.size());
  std::vector<int> smallest(clusters.size());
  for (size_t c = 0; c < clusters.size(); c++) { order[c] = c; smallest[c] = *std::min_element(clusters[c].begin(), clusters[c].end()); }
  std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return smallest[x] < smallest[y]; });
  for (size_t q = 0; q < order.size(); q++) rank[order[q]] = q;
  FILE* fp = open_out(output, "print_upgma_newick");
  for (size_t c = 0; c < clusters.size(); c++) {
    const size_t q = rank[c];
    std::vector<uint32_t> mem(clusters[c].begin(), clusters[c].end());
    std::sort(mem.begin(), mem.end());
    fprintf(fp, "%s\n", upgma_newick_text([&](uint32_t v) { return sketchByFile ? g[v].fileName : g[v].seq0.name; }, mem.data(), mem.size(),
                                          merges.data() + first[q], (size_t)(first[q + 1] - first[q])).c_str());
  }
  fclose(fp);
}

double quality_report_text(const std::function<std::string(uint32_t)>& name, const std::vector<std::vector<int>>& clusters, const rtc_sil* rec,
                           const double* sil, uint32_t n, std::string* quality_tsv, std::string* silhouette_tsv) {
  char buf[512];
  std::vector<int32_t> label(n, -1);
  std::string& Q = *quality_tsv;
  Q = "cluster\tsize\tmean_silhouette\tmin_silhouette\tmean_intra_distance\tdiameter\tseparation\tnearest_cluster\n";
  for (size_t c = 0; c < clusters.size(); c++) {
    std::vector<int> mem(clusters[c]);
    std::sort(mem.begin(), mem.end());
    const size_t sz = mem.size();
    double sum = 0.0, least = 0.0;
    uint64_t a_total = 0;
    uint32_t far = 0, near = 1u << 20, near_cluster = 0xffffffffu;
    for (size_t i = 0; i < sz; i++) {
      const rtc_sil& r = rec[mem[i]];
      label[mem[i]] = (int32_t)c;
      sum += sil[mem[i]];
      if (i == 0 || sil[mem[i]] < least) least = sil[mem[i]];
      a_total += r.a_num;
      if (r.far_q > far) far = r.far_q;
      if (i == 0 || r.near_q < near) { near = r.near_q; near_cluster = r.near_cluster; }
    }
    const double mean = sz ? sum / (double)sz : 0.0;
    const double intra = sz > 1 ? (double)a_total / ((double)sz * (double)(sz - 1) * 1048576.0) : 0.0;
    snprintf(buf, sizeof buf, "%zu\t%zu\t%.6f\t%.6f\t%.6f\t%.6f\t%.6f\t", c, sz, mean, least, intra, (double)far / 1048576.0, (double)near / 1048576.0);
    Q += buf;
    Q += near_cluster == 0xffffffffu ? std::string("-") : std::to_string(near_cluster);
    Q += "\n";
  }
  double all = 0.0;
  for (uint32_t g = 0; g < n; g++) all += sil[g];
  const double all_mean = n ? all / (double)n : 0.0;
  snprintf(buf, sizeof buf, "all\t%u\t%.6f\t-\t-\t-\t-\t-\n", n, all_mean);
  Q += buf;
  std::string& S = *silhouette_tsv;
  S = "name\tcluster\tsilhouette\ta\tb\tb_cluster\n";
  for (uint32_t g = 0; g < n; g++) {
    const rtc_sil& r = rec[g];
    const double a = r.a_den ? (double)r.a_num / ((double)r.a_den * 1048576.0) : 0.0;
    const double b = r.b_den ? (double)r.b_num / ((double)r.b_den * 1048576.0) : 0.0;
    snprintf(buf, sizeof buf, "\t%d\t%.6f\t%.6f\t%.6f\t", label[g], sil[g], a, b);
    S += name(g);
    S += buf;
    S += r.b_cluster == 0xffffffffu ? std::string("-") : std::to_string(r.b_cluster);
    S += "\n";
  }
  return all_mean;
}

double support_report_text(const std::function<std::string(uint32_t)>& name, const std::vector<std::vector<int>>& clusters, const rtc_csupport* rec,
                           const uint64_t* together, uint32_t n, uint32_t replicates, std::string* support_tsv, std::string* genomes_tsv) {
  char buf[512];
  const size_t nc = clusters.size();
  // the library numbers the clusters by their smallest member
  std::vector<size_t> order(nc), rank(nc);
  std::vector<int> smallest(nc, 0);
  for (size_t c = 0; c < nc; c++) { order[c] = c; if (!clusters[c].empty()) smallest[c] = *std::min_element(clusters[c].begin(), clusters[c].end()); }
  std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return smallest[x] < smallest[y]; });
  for (size_t q = 0; q < nc; q++) rank[order[q]] = q;
  std::vector<int32_t> label(n, -1);
  std::string& S = *support_tsv;
  S = "cluster\tsize\treplicates\trecovered\tsplit\tmerged\tmixed\tmax_pieces\tsupport\n";
  uint64_t recovered = 0;
  for (size_t c = 0; c < nc; c++) {
    const rtc_csupport& r = rec[rank[c]];
    for (int g : clusters[c]) label[g] = (int32_t)c;
    recovered += r.recovered;
    snprintf(buf, sizeof buf, "%zu\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\n", c, r.size, replicates, r.recovered, r.split, r.merged, r.mixed, r.max_pieces,
             nj_support_percent(r.recovered, replicates));
    S += buf;
  }
  std::string& G = *genomes_tsv;
  G = "name\tcluster\ttogether\tfraction\n";
  for (uint32_t g = 0; g < n; g++) {
    const size_t size = label[g] >= 0 ? clusters[label[g]].size() : 0;
    snprintf(buf, sizeof buf, "\t%d\t%llu\t", label[g], (unsigned long long)together[g]);
    G += name(g);
    G += buf;
    if (size > 1) {
      snprintf(buf, sizeof buf, "%.6f", (double)together[g] / ((double)replicates * (double)(size - 1)));
      G += buf;
    } else {
      G += "-";
    }
    G += "\n";
  }
  return nc ? (double)recovered / (double)nc : 0.0;
}

double pangenome_report_text(const std::function<std::string(uint32_t)>& name, const std::vector<std::vector<int>>& clusters, const rtc_pan* rec,
                             const uint64_t* hist, const rtc_pan_genome* gen, uint32_t n, int threads, pan_growth_fn growth_fn, std::string* pan_tsv,
                             std::string* genomes_tsv, std::string* hist_tsv, std::string* curve_tsv) {
  char buf[512];
  const size_t nc = clusters.size();
  // the library numbers the clusters by their smallest member; a cluster's histogram starts behind those of the clusters before it
  std::vector<size_t> order(nc), rank(nc);
  std::vector<int> smallest(nc, 0);
  for (size_t c = 0; c < nc; c++) { order[c] = c; if (!clusters[c].empty()) smallest[c] = *std::min_element(clusters[c].begin(), clusters[c].end()); }
  std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return smallest[x] < smallest[y]; });
  for (size_t q = 0; q < nc; q++) rank[order[q]] = q;
  std::vector<uint64_t> first(nc + 1, 0);
  for (size_t q = 0; q < nc; q++) first[q + 1] = first[q] + rec[q].size;
  std::vector<int32_t> label(n, -1);
  std::string &P = *pan_tsv, &H = *hist_tsv, &V = *curve_tsv;
  P = "cluster\tsize\thashes\tpan\tcore\tsoft_core\tshell\tcloud\tsingletons\tcore_share\tnew_per_genome\tcentre\n";
  H = "cluster\tf\tcount\n";
  V = "cluster\tj\tpan\tcore\n";
  double share_sum = 0.0;
  size_t share_n = 0;
  std::vector<uint32_t> js;
  std::vector<double> gp, gc;
  for (size_t c = 0; c < nc; c++) {
    const rtc_pan& r = rec[rank[c]];
    const uint64_t* h = hist + first[rank[c]];
    int centre = -1;
    for (int g : clusters[c]) {
      label[g] = (int32_t)c;
      if (centre < 0 || gen[g].occ_sum > gen[centre].occ_sum || (gen[g].occ_sum == gen[centre].occ_sum && g < centre)) centre = g;
    }
    snprintf(buf, sizeof buf, "%zu\t%u\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t", c, r.size, (unsigned long long)r.total, (unsigned long long)r.pan,
             (unsigned long long)r.core, (unsigned long long)r.soft, (unsigned long long)r.shell, (unsigned long long)r.cloud,
             (unsigned long long)r.single);
    P += buf;
    if (r.pan) {
      const double share = (double)r.core / (double)r.pan;
      share_sum += share;
      share_n++;
      snprintf(buf, sizeof buf, "%.6f", share);
      P += buf;
    } else {
      P += "-";
    }
    snprintf(buf, sizeof buf, "\t%.6f\t", r.size ? (double)h[0] / (double)r.size : 0.0);
    P += buf;
    P += centre >= 0 ? name((uint32_t)centre) : std::string("-");
    P += "\n";
    for (uint32_t f = 1; f <= r.size; f++)
      if (h[f - 1]) {
        snprintf(buf, sizeof buf, "%zu\t%u\t%llu\n", c, f, (unsigned long long)h[f - 1]);
        H += buf;
      }
    if (r.size >= 2 && growth_fn) {
      const uint32_t cap = r.size < 256 ? r.size : 256;
      js.assign(cap, 0); gp.assign(cap, 0.0); gc.assign(cap, 0.0);
      uint32_t points = 0;
      if (growth_fn(h, r.size, threads, js.data(), gp.data(), gc.data(), &points) == 0)
        for (uint32_t p = 0; p < points && p < cap; p++) {
          snprintf(buf, sizeof buf, "%zu\t%u\t%.6f\t%.6f\n", c, js[p], gp[p], gc[p]);
          V += buf;
        }
    }
  }
  std::string& G = *genomes_tsv;
  G = "name\tcluster\thashes\tunique\tcore\tsoft_core\tshell\tcloud\ttypicality\n";
  for (uint32_t g = 0; g < n; g++) {
    const rtc_pan_genome& r = gen[g];
    const uint64_t hashes = (uint64_t)r.core + r.soft + r.shell + r.cloud;  // every hash of a clustered genome has a class
    const size_t size = label[g] >= 0 ? clusters[label[g]].size() : 0;
    snprintf(buf, sizeof buf, "\t%d\t%llu\t%u\t%u\t%u\t%u\t%u\t", label[g], (unsigned long long)hashes, r.unique, r.core, r.soft, r.shell, r.cloud);
    G += name(g);
    G += buf;
    if (hashes && size) {
      snprintf(buf, sizeof buf, "%.6f", (double)r.occ_sum / ((double)hashes * (double)size));
      G += buf;
    } else {
      G += "-";
    }
    G += "\n";
  }
  return share_n ? share_sum / (double)share_n : 0.0;
}

void print_phylip_tree(const std::vector<GenomeInfo>& g, const std::vector<rtc_edge>& mst, bool sketchByFile, const std::string& output) {
  FILE* fp = open_out(output, "print_phylip_tree");
  fprintf(fp, "1\n%s\n", get_newick_tree(g, mst, sketchByFile).c_str());
  fclose(fp);
}

void print_nexus_tree(const std::vector<GenomeInfo>& g, const std::vector<rtc_edge>& mst, bool sketchByFile, const std::string& output) {  // src/MST_IO.cpp:296-335
  const std::string tree = get_newick_tree(g, mst, sketchByFile);
  FILE* fp = open_out(output, "print_nexus_tree");
  fprintf(fp, "#NEXUS\nBEGIN TAXA;\n  DIMENSIONS NTAX=%zu;\n  TAXLABELS", g.size());
  for (const GenomeInfo& gi : g) {
    std::string lab = sketchByFile ? gi.fileName : gi.seq0.name;
    size_t pos = 0;
    while ((pos = lab.find('\'', pos)) != std::string::npos) { lab.insert(pos, "'"); pos += 2; }  // quotes are doubled
    fprintf(fp, " '%s'", lab.c_str());
  }
  fprintf(fp, ";\nEND;\nBEGIN TREES;\n  TREE tree_1 = [&R] %s\nEND;\n", tree.c_str());
  fclose(fp);
}

void print_linkage_matrix(int N, const std::vector<rtc_edge>& mst, const std::string& output) {  // src/MST.cpp:1246-1287, src/MST_IO.cpp:362-376
  FILE* fp = open_out(output, "print_linkage_matrix");
  if (N > 1) {
    const std::vector<rtc_edge> edges = by_distance(mst);
    DSU dsu(N);
    int next_id = N;
    std::vector<int> cluster_id(N), cluster_size(2 * N - 1);
    for (int i = 0; i < N; i++) { cluster_id[i] = i; cluster_size[i] = 1; }
    for (const rtc_edge& e : edges) {
      const int ru = dsu.find(e.preNode), rv = dsu.find(e.sufNode);
      if (ru == rv) continue;
      const int id_u = cluster_id[ru], id_v = cluster_id[rv];
      const int new_id = next_id++, new_size = cluster_size[id_u] + cluster_size[id_v];
      fprintf(fp, "%d\t%d\t%.6f\t%d\n", id_u, id_v, e.dist, new_size);
      cluster_id[dsu.unite(ru, rv)] = new_id;
      cluster_size[new_id] = new_size;
    }
  }
  fclose(fp);
}

std::vector<rtc_edge> kruskal_algorithm(const std::vector<rtc_edge>& graph, int vertices) {  // src/MST.cpp:59-75
  std::vector<int> parent(vertices), ranks(vertices, 0);             // UnionFind.h: union by rank, path compression
  for (int v = 0; v < vertices; v++) parent[v] = v;
  auto find = [&](int x) { int r = x; while (parent[r] != r) r = parent[r]; while (parent[x] != r) { int nx = parent[x]; parent[x] = r; x = nx; } return r; };
  std::vector<rtc_edge> tree;
  for (const rtc_edge& e : graph) {
    int a = find(e.preNode), b = find(e.sufNode);
    if (a == b) continue;
    if (ranks[a] > ranks[b]) parent[b] = a;
    else if (ranks[a] < ranks[b]) parent[a] = b;
    else { parent[a] = b; ranks[b]++; }
    tree.push_back(e);
  }
  return tree;
}

std::vector<rtc_edge> generate_forest(const std::vector<rtc_edge>& mst, double threshold) {  // src/MST.cpp:77-85
  std::vector<rtc_edge> forest;
  for (const rtc_edge& e : mst) if (e.dist <= threshold) forest.push_back(e);
  return forest;
}

std::vector<std::vector<int>> generate_cluster_with_bfs(const std::vector<rtc_edge>& forest, int vertices) {  // :109-142
  std::vector<std::vector<int>> res, G(vertices);
  for (const rtc_edge& e : forest) { G[e.preNode].push_back(e.sufNode); G[e.sufNode].push_back(e.preNode); }
  std::vector<char> visited(vertices, 0);
  for (int i = 0; i < vertices; i++) {
    if (visited[i]) continue;
    visited[i] = 1;
    std::queue<int> Q; Q.push(i);
    std::vector<int> cl{i};
    while (!Q.empty()) {
      int k = Q.front(); Q.pop();
      for (int v : G[k]) { if (visited[v]) continue; visited[v] = 1; Q.push(v); cl.push_back(v); }
    }
    res.push_back(std::move(cl));
  }
  return res;
}

// skips n bytes of fp; false when the file ends before them
static bool skip_bytes(FILE* fp, size_t n) {
  const long at = ftell(fp);
  if (at < 0 || fseek(fp, 0, SEEK_END) != 0) return false;
  const long end = ftell(fp);
  if (end < 0 || (size_t)(end - at) < n) return false;
  return fseek(fp, at + (long)n, SEEK_SET) == 0;
}

// the representatives' inverted index as the reference's writers lay it out (hash, list length, positions in
// rep_ids); keys ascending here (the reference walks a hash map)
static size_t write_rep_index(FILE* fp, const KssdClusterState& st) {
  std::vector<std::pair<uint64_t, int>> post;
  const size_t rep_count = st.reps.use64 ? st.reps.h64.size() : st.reps.h32.size();
  for (size_t r = 0; r < rep_count; r++) {
    if (st.reps.use64) for (uint64_t h : st.reps.h64[r]) post.emplace_back(h, (int)r);
    else for (uint32_t h : st.reps.h32[r]) post.emplace_back((uint64_t)h, (int)r);
  }
  std::sort(post.begin(), post.end());
  size_t index_size = 0;
  for (size_t i = 0; i < post.size(); i++) if (i == 0 || post[i].first != post[i - 1].first) index_size++;
  wr(fp, index_size);
  for (size_t i = 0; i < post.size();) {
    size_t j = i;
    while (j < post.size() && post[j].first == post[i].first) j++;
    wr(fp, post[i].first);
    const size_t list_size = j - i;
    wr(fp, list_size);
    for (size_t q = i; q < j; q++) wr(fp, post[q].second);
    i = j;
  }
  return index_size;
}

static void write_state_sketch(FILE* fp, const GenomeInfo& g, const KssdSketchFile& sk, size_t i) {
  const bool use64 = sk.use64;
  const size_t n32 = use64 ? 0 : sk.h32[i].size(), n64 = use64 ? sk.h64[i].size() : 0;
  const uint32_t sketchsize = (uint32_t)(n32 + n64);
  wr(fp, g.id); wr(fp, g.totalSeqLength); wr(fp, use64); wr(fp, sketchsize);
  wr(fp, n32); wr(fp, n64);
  if (n32) fwrite(sk.h32[i].data(), 4, n32, fp);
  if (n64) fwrite(sk.h64[i].data(), 8, n64, fp);
  const size_t name_len = g.fileName.size();
  wr(fp, name_len);
  fwrite(g.fileName.data(), 1, name_len, fp);
}

static bool read_state_sketch(FILE* fp, GenomeInfo& g, KssdSketchFile& sk, bool first) {
  bool use64 = false; uint32_t sketchsize = 0; size_t n32 = 0, n64 = 0, name_len = 0;
  bool ok = rd(fp, g.id) && rd(fp, g.totalSeqLength) && rd(fp, use64) && rd(fp, sketchsize) && rd(fp, n32) && rd(fp, n64) &&
            n32 < ((size_t)1 << 32) && n64 < ((size_t)1 << 32);
  if (!ok) return false;
  if (first) sk.use64 = use64;
  std::vector<uint32_t> h32(n32); std::vector<uint64_t> h64(n64);
  if (n32) ok = ok && fread(h32.data(), 4, n32, fp) == n32;
  if (n64) ok = ok && fread(h64.data(), 8, n64, fp) == n64;
  ok = ok && rd(fp, name_len) && name_len < ((size_t)1 << 20);
  if (!ok) return false;
  g.fileName.resize(name_len);
  if (name_len) ok = fread(&g.fileName[0], 1, name_len, fp) == name_len;
  g.use64 = use64;
  g.seq0.name = "N/A"; g.seq0.comment = "N/A";   // printKssdResult's text for sketches without record infos (src/MST_IO.cpp:99-104)
  if (sk.use64) sk.h64.push_back(std::move(h64)); else sk.h32.push_back(std::move(h32));
  return ok;
}

// src/MST_IO.cpp:72-179 (printResult / printKssdResult share the layout)
// src/greedy.cpp:1545-1625
bool save_kssd_cluster_state(const std::string& path, const KssdClusterState& st) {
  FILE* fp = fopen(path.c_str(), "wb");
  if (!fp) { std::cerr << "ERROR: Cannot open file for writing: " << path << std::endl; return false; }
  wr(fp, st.threshold); wr(fp, st.kmer_size);
  wr(fp, st.info.half_k); wr(fp, st.info.half_subk); wr(fp, st.info.drlevel); wr(fp, st.info.genomeNumber);
  const size_t rep_count = st.rep_ids.size();
  wr(fp, rep_count);
  fwrite(st.rep_ids.data(), sizeof(int), rep_count, fp);
  const size_t sketch_count = st.genomes.size();
  wr(fp, sketch_count);
  for (size_t i = 0; i < sketch_count; i++) write_state_sketch(fp, st.genomes[i], st.sk, i);
  const size_t cluster_count = st.clusters.size();
  wr(fp, cluster_count);
  for (const auto& c : st.clusters) {
    const size_t m = c.size();
    wr(fp, m);
    fwrite(c.data(), sizeof(int), m, fp);
  }
  // representatives' inverted index: marker + 64-bit keys
  const char magic[8] = {'K', 'S', 'S', 'I', '0', '2', '\0', '\0'};
  fwrite(magic, 1, 8, fp);
  const size_t index_size = write_rep_index(fp, st);
  fclose(fp);
  std::cerr << "Saved clustering state to: " << path << std::endl
            << "  - " << sketch_count << " genomes" << std::endl
            << "  - " << rep_count << " clusters (representatives)" << std::endl
            << "  - " << index_size << " unique hashes in inverted index" << std::endl;
  return true;
}

// MinHashClusterState::save (src/greedy.cpp:2134-2208): "MINHASH\0", threshold, k, sketch size, containment flag,
// representative ids, every sketch in clustering order {id, length, hashes, file name}, the clusters (members are
// positions in that order, the representative first), the representatives' inverted index hash -> positions in
// representative_ids.  The reference writes the index in hash-map iteration order; here ascending by hash (readers
// rebuild a map from it either way).
bool save_minhash_cluster_state(const std::string& path, const KssdClusterState& st) {
  FILE* fp = fopen(path.c_str(), "wb");
  if (!fp) { std::cerr << "ERROR: Cannot open file for writing: " << path << std::endl; return false; }
  const char magic[8] = {'M', 'I', 'N', 'H', 'A', 'S', 'H', '\0'};
  fwrite(magic, 1, 8, fp);
  wr(fp, st.threshold); wr(fp, st.kmer_size); wr(fp, st.sketch_size); wr(fp, st.is_containment);
  const size_t rep_count = st.rep_ids.size();
  wr(fp, rep_count);
  fwrite(st.rep_ids.data(), sizeof(int), rep_count, fp);
  const size_t sketch_count = st.genomes.size();
  wr(fp, sketch_count);
  for (size_t i = 0; i < sketch_count; i++) {
    const GenomeInfo& g = st.genomes[i];
    wr(fp, g.id); wr(fp, g.totalSeqLength);
    const size_t hash_count = st.sk.h64[i].size();
    wr(fp, hash_count);
    if (hash_count) fwrite(st.sk.h64[i].data(), 8, hash_count, fp);
    const size_t name_len = g.fileName.size();
    wr(fp, name_len);
    fwrite(g.fileName.data(), 1, name_len, fp);
  }
  const size_t cluster_count = st.clusters.size();
  wr(fp, cluster_count);
  for (const auto& c : st.clusters) {
    const size_t m = c.size();
    wr(fp, m);
    fwrite(c.data(), sizeof(int), m, fp);
  }
  std::cerr << "Saving inverted index: ";
  const size_t index_size = write_rep_index(fp, st);
  std::cerr << index_size << " unique hashes..." << std::endl;
  fclose(fp);
  std::cerr << "Saved clustering state to: " << path << std::endl
            << "  - " << sketch_count << " genomes" << std::endl
            << "  - " << rep_count << " clusters (representatives)" << std::endl
            << "  - " << index_size << " unique hashes in inverted index" << std::endl;
  return true;
}

// MinHashClusterState::load (src/greedy.cpp:2210-2302): parameters, representative ids and clusters are kept; the
// sketches are skipped (the caller reloads them from the folder, src/sub_command.cpp:100-139) and so is the index
// (it is rebuilt from the representatives).
bool load_minhash_cluster_state(const std::string& path, KssdClusterState& st) {
  FILE* fp = fopen(path.c_str(), "rb");
  if (!fp) { std::cerr << "ERROR: Cannot open file for reading: " << path << std::endl; return false; }
  char magic[8] = {0};
  if (fread(magic, 1, 8, fp) != 8 || strncmp(magic, "MINHASH", 8) != 0) {
    std::cerr << "ERROR: Invalid file format (not a MinHash cluster state)" << std::endl;
    fclose(fp);
    return false;
  }
  st = KssdClusterState();
  st.minhash = true; st.sk.use64 = true; st.reps.use64 = true;
  bool ok = rd(fp, st.threshold) && rd(fp, st.kmer_size) && rd(fp, st.sketch_size) && rd(fp, st.is_containment);
  size_t rep_count = 0, sketch_count = 0, cluster_count = 0;
  ok = ok && rd(fp, rep_count) && rep_count < ((size_t)1 << 31);
  if (ok) { st.rep_ids.resize(rep_count); ok = fread(st.rep_ids.data(), sizeof(int), rep_count, fp) == rep_count; }
  ok = ok && rd(fp, sketch_count) && sketch_count < ((size_t)1 << 31);
  for (size_t i = 0; ok && i < sketch_count; i++) {
    int id; uint64_t len; size_t hash_count = 0, name_len = 0;
    ok = rd(fp, id) && rd(fp, len) && rd(fp, hash_count) && hash_count < ((size_t)1 << 32) &&
         fseek(fp, (long)(hash_count * 8), SEEK_CUR) == 0 && rd(fp, name_len) && name_len < ((size_t)1 << 20) &&
         fseek(fp, (long)name_len, SEEK_CUR) == 0;
  }
  ok = ok && rd(fp, cluster_count) && cluster_count < ((size_t)1 << 31);
  for (size_t c = 0; ok && c < cluster_count; c++) {
    size_t m = 0;
    ok = rd(fp, m) && m < ((size_t)1 << 31);
    if (!ok) break;
    std::vector<int> cl(m);
    if (m) ok = fread(cl.data(), sizeof(int), m, fp) == m;
    st.clusters.push_back(std::move(cl));
  }
  size_t index_size = 0;
  ok = ok && rd(fp, index_size);
  fclose(fp);
  if (!ok) { std::cerr << "ERROR: truncated or malformed cluster state: " << path << std::endl; return false; }
  std::cerr << "Loading inverted index: " << index_size << " unique hashes..." << std::endl;
  std::cerr << "Loaded clustering state from: " << path << std::endl
            << "  - " << sketch_count << " genomes" << std::endl
            << "  - " << rep_count << " clusters (representatives)" << std::endl
            << "  - " << index_size << " unique hashes in inverted index" << std::endl;
  return true;
}

// src/greedy.cpp:1627-1734 (the inverted index that follows the clusters is not read: it is a function of the
// representatives' sketches)
bool load_kssd_cluster_state(const std::string& path, KssdClusterState& st) {
  FILE* fp = fopen(path.c_str(), "rb");
  if (!fp) { std::cerr << "ERROR: Cannot open file for reading: " << path << std::endl; return false; }
  bool ok = rd(fp, st.threshold) && rd(fp, st.kmer_size) && rd(fp, st.info.half_k) && rd(fp, st.info.half_subk) &&
            rd(fp, st.info.drlevel) && rd(fp, st.info.genomeNumber);
  size_t rep_count = 0, sketch_count = 0, cluster_count = 0;
  ok = ok && rd(fp, rep_count) && rep_count < ((size_t)1 << 31);
  if (ok) { st.rep_ids.resize(rep_count); ok = fread(st.rep_ids.data(), sizeof(int), rep_count, fp) == rep_count; }
  ok = ok && rd(fp, sketch_count) && sketch_count < ((size_t)1 << 31);
  st.genomes.clear(); st.sk.h32.clear(); st.sk.h64.clear(); st.sk.info = st.info;
  for (size_t i = 0; ok && i < sketch_count; i++) {
    GenomeInfo g;
    ok = read_state_sketch(fp, g, st.sk, i == 0);
    if (ok) st.genomes.push_back(g);
  }
  ok = ok && rd(fp, cluster_count) && cluster_count < ((size_t)1 << 31);
  st.clusters.clear();
  for (size_t c = 0; ok && c < cluster_count; c++) {
    size_t m = 0;
    ok = rd(fp, m) && m < ((size_t)1 << 31);
    if (!ok) break;
    std::vector<int> cl(m);
    if (m) ok = fread(cl.data(), sizeof(int), m, fp) == m;
    st.clusters.push_back(std::move(cl));
  }
  fclose(fp);
  if (!ok) { std::cerr << "ERROR: truncated or malformed cluster state: " << path << std::endl; return false; }
  for (int r : st.rep_ids) if (r < 0 || (size_t)r >= st.genomes.size()) { std::cerr << "ERROR: Representative ID " << r << " out of range" << std::endl; return false; }
  if (st.clusters.size() != rep_count) { std::cerr << "ERROR: " << st.clusters.size() << " clusters for " << rep_count << " representatives" << std::endl; return false; }
  st.reps = KssdSketchFile(); st.reps.info = st.info; st.reps.use64 = st.sk.use64; st.rep_genomes.clear();
  for (int r : st.rep_ids) {   // representatives = all_sketches[representative_ids] (src/greedy.cpp:1676-1685)
    st.rep_genomes.push_back(st.genomes[r]);
    if (st.sk.use64) st.reps.h64.push_back(st.sk.h64[r]); else st.reps.h32.push_back(st.sk.h32[r]);
  }
  std::cerr << "Loaded clustering state from: " << path << std::endl
            << "  - " << sketch_count << " genomes" << std::endl
            << "  - " << rep_count << " clusters (representatives)" << std::endl;
  return true;
}

// src/greedy.cpp:2351-2428
bool save_kssd_repdb(const std::string& path, const KssdClusterState& st) {
  FILE* fp = fopen(path.c_str(), "wb");
  if (!fp) { std::cerr << "ERROR: Cannot open RepDB file for writing: " << path << std::endl; return false; }
  fwrite("REPDB002", 1, 8, fp);
  wr(fp, st.threshold); wr(fp, st.kmer_size);
  wr(fp, st.info.half_k); wr(fp, st.info.half_subk); wr(fp, st.info.drlevel); wr(fp, st.info.genomeNumber);
  const size_t rep_count = st.rep_ids.size();
  wr(fp, rep_count);
  for (size_t r = 0; r < rep_count; r++) {
    wr(fp, st.rep_ids[r]);
    write_state_sketch(fp, st.rep_genomes[r], st.reps, r);
  }
  const size_t cluster_count = st.clusters.size();
  wr(fp, cluster_count);
  for (const auto& c : st.clusters) {
    const size_t m = c.size();
    wr(fp, m);
    fwrite(c.data(), sizeof(int), m, fp);
  }
  const size_t all_count = st.genomes.size();
  wr(fp, all_count);
  for (const GenomeInfo& g : st.genomes) {
    const size_t name_len = g.fileName.size();
    wr(fp, name_len);
    fwrite(g.fileName.data(), 1, name_len, fp);
    wr(fp, g.totalSeqLength);
  }
  const size_t index_size = write_rep_index(fp, st);
  fclose(fp);
  std::cerr << "RepDB saved to: " << path << std::endl
            << "  Representatives: " << rep_count << std::endl
            << "  Total genomes:   " << all_count << std::endl
            << "  Inverted index:  " << index_size << " unique hashes" << std::endl;
  return true;
}

// src/greedy.cpp:2430-2537
bool load_kssd_repdb(const std::string& path, KssdClusterState& st) {
  FILE* fp = fopen(path.c_str(), "rb");
  if (!fp) { std::cerr << "ERROR: Cannot open RepDB file for reading: " << path << std::endl; return false; }
  char magic[8] = {0};
  if (fread(magic, 1, 8, fp) != 8 || (memcmp(magic, "REPDB002", 8) != 0 && memcmp(magic, "REPDB001", 8) != 0)) {
    std::cerr << "ERROR: Invalid RepDB file (bad magic): " << path << std::endl;
    fclose(fp);
    return false;
  }
  const bool v2 = memcmp(magic, "REPDB002", 8) == 0;
  bool ok = rd(fp, st.threshold) && rd(fp, st.kmer_size) && rd(fp, st.info.half_k) && rd(fp, st.info.half_subk) &&
            rd(fp, st.info.drlevel) && rd(fp, st.info.genomeNumber);
  size_t rep_count = 0, cluster_count = 0, all_count = 0, index_size = 0;
  ok = ok && rd(fp, rep_count) && rep_count < ((size_t)1 << 31);
  st.rep_ids.clear(); st.rep_genomes.clear(); st.genomes.clear(); st.clusters.clear();
  st.sk = KssdSketchFile(); st.reps = KssdSketchFile(); st.reps.info = st.info; st.sk.info = st.info;
  for (size_t r = 0; ok && r < rep_count; r++) {
    int rid = 0; GenomeInfo g;
    ok = rd(fp, rid) && read_state_sketch(fp, g, st.reps, r == 0);
    if (ok) { st.rep_ids.push_back(rid); st.rep_genomes.push_back(g); }
  }
  st.sk.use64 = st.reps.use64;
  ok = ok && rd(fp, cluster_count) && cluster_count < ((size_t)1 << 31);
  for (size_t c = 0; ok && c < cluster_count; c++) {
    size_t m = 0;
    ok = rd(fp, m) && m < ((size_t)1 << 31);
    if (!ok) break;
    std::vector<int> cl(m);
    if (m) ok = fread(cl.data(), sizeof(int), m, fp) == m;
    st.clusters.push_back(std::move(cl));
  }
  ok = ok && rd(fp, all_count) && all_count < ((size_t)1 << 31);
  for (size_t i = 0; ok && i < all_count; i++) {
    GenomeInfo g; size_t name_len = 0;
    ok = rd(fp, name_len) && name_len < ((size_t)1 << 20);
    if (!ok) break;
    g.fileName.resize(name_len);
    if (name_len) ok = fread(&g.fileName[0], 1, name_len, fp) == name_len;
    ok = ok && rd(fp, g.totalSeqLength);
    g.id = 0; g.use64 = st.reps.use64;   // load_repdb fills only the name and the length of all_sketches
    g.seq0.name = "N/A"; g.seq0.comment = "N/A";
    st.genomes.push_back(g);
  }
  ok = ok && rd(fp, index_size);
  for (size_t i = 0; ok && i < index_size; i++) {   // walked for the truncation check only
    uint64_t h64 = 0; uint32_t h32 = 0; size_t ls = 0;
    ok = (v2 ? rd(fp, h64) : rd(fp, h32)) && rd(fp, ls) && ls < ((size_t)1 << 31) && skip_bytes(fp, ls * sizeof(int));
  }
  fclose(fp);
  if (!ok) { std::cerr << "ERROR: truncated or malformed RepDB: " << path << std::endl; return false; }
  if (st.clusters.size() != rep_count) { std::cerr << "ERROR: " << st.clusters.size() << " clusters for " << rep_count << " representatives" << std::endl; return false; }
  std::cerr << "RepDB loaded from: " << path << std::endl
            << "  Representatives: " << rep_count << std::endl
            << "  Total genomes:   " << all_count << std::endl
            << "  Inverted index:  " << index_size << " unique hashes" << std::endl
            << "  Threshold:       " << st.threshold << std::endl
            << "  Kmer size:       " << st.kmer_size << std::endl;
  return true;
}

// src/greedy.cpp:2789-2862
bool save_minhash_repdb(const std::string& path, const KssdClusterState& st) {
  FILE* fp = fopen(path.c_str(), "wb");
  if (!fp) { std::cerr << "ERROR: Cannot open RepDB file for writing: " << path << std::endl; return false; }
  fwrite("MHREPDB1", 1, 8, fp);
  wr(fp, st.threshold); wr(fp, st.kmer_size); wr(fp, st.sketch_size); wr(fp, st.is_containment);
  const size_t rep_count = st.rep_ids.size();
  wr(fp, rep_count);
  for (size_t r = 0; r < rep_count; r++) {
    const GenomeInfo& g = st.rep_genomes[r];
    wr(fp, st.rep_ids[r]); wr(fp, g.id); wr(fp, g.totalSeqLength); wr(fp, st.is_containment);
    const size_t hash_count = st.reps.h64[r].size();
    wr(fp, hash_count);
    if (hash_count) fwrite(st.reps.h64[r].data(), 8, hash_count, fp);
    const size_t name_len = g.fileName.size();
    wr(fp, name_len);
    fwrite(g.fileName.data(), 1, name_len, fp);
  }
  const size_t cluster_count = st.clusters.size();
  wr(fp, cluster_count);
  for (const auto& c : st.clusters) {
    const size_t m = c.size();
    wr(fp, m);
    fwrite(c.data(), sizeof(int), m, fp);
  }
  const size_t all_count = st.genomes.size();
  wr(fp, all_count);
  for (const GenomeInfo& g : st.genomes) {
    const size_t name_len = g.fileName.size();
    wr(fp, name_len);
    fwrite(g.fileName.data(), 1, name_len, fp);
    wr(fp, g.totalSeqLength);
  }
  const size_t index_size = write_rep_index(fp, st);
  fclose(fp);
  std::cerr << "MinHash RepDB saved to: " << path << std::endl
            << "  Representatives: " << rep_count << std::endl
            << "  Total genomes:   " << all_count << std::endl
            << "  Inverted index:  " << index_size << " unique hashes" << std::endl;
  return true;
}

// src/greedy.cpp:2864-2956
bool load_minhash_repdb(const std::string& path, KssdClusterState& st) {
  FILE* fp = fopen(path.c_str(), "rb");
  if (!fp) { std::cerr << "ERROR: Cannot open RepDB file for reading: " << path << std::endl; return false; }
  char magic[8] = {0};
  if (fread(magic, 1, 8, fp) != 8 || memcmp(magic, "MHREPDB1", 8) != 0) {
    std::cerr << "ERROR: Invalid MinHash RepDB file (bad magic): " << path << std::endl;
    fclose(fp);
    return false;
  }
  st = KssdClusterState();
  st.minhash = true; st.reps.use64 = true; st.sk.use64 = true;
  bool ok = rd(fp, st.threshold) && rd(fp, st.kmer_size) && rd(fp, st.sketch_size) && rd(fp, st.is_containment);
  size_t rep_count = 0, cluster_count = 0, all_count = 0, index_size = 0;
  ok = ok && rd(fp, rep_count) && rep_count < ((size_t)1 << 31);
  for (size_t r = 0; ok && r < rep_count; r++) {
    int rid = 0; GenomeInfo g; bool cont = false; size_t hash_count = 0, name_len = 0;
    ok = rd(fp, rid) && rd(fp, g.id) && rd(fp, g.totalSeqLength) && rd(fp, cont) && rd(fp, hash_count) && hash_count < ((size_t)1 << 32);
    if (!ok) break;
    std::vector<uint64_t> h(hash_count);
    if (hash_count) ok = fread(h.data(), 8, hash_count, fp) == hash_count;
    ok = ok && rd(fp, name_len) && name_len < ((size_t)1 << 20);
    if (!ok) break;
    g.fileName.resize(name_len);
    if (name_len) ok = fread(&g.fileName[0], 1, name_len, fp) == name_len;
    g.seq0.name = "N/A"; g.seq0.comment = "";
    st.rep_ids.push_back(rid); st.rep_genomes.push_back(g); st.reps.h64.push_back(std::move(h));
  }
  ok = ok && rd(fp, cluster_count) && cluster_count < ((size_t)1 << 31);
  for (size_t c = 0; ok && c < cluster_count; c++) {
    size_t m = 0;
    ok = rd(fp, m) && m < ((size_t)1 << 31);
    if (!ok) break;
    std::vector<int> cl(m);
    if (m) ok = fread(cl.data(), sizeof(int), m, fp) == m;
    st.clusters.push_back(std::move(cl));
  }
  ok = ok && rd(fp, all_count) && all_count < ((size_t)1 << 31);
  for (size_t i = 0; ok && i < all_count; i++) {
    GenomeInfo g; size_t name_len = 0;
    ok = rd(fp, name_len) && name_len < ((size_t)1 << 20);
    if (!ok) break;
    g.fileName.resize(name_len);
    if (name_len) ok = fread(&g.fileName[0], 1, name_len, fp) == name_len;
    ok = ok && rd(fp, g.totalSeqLength);
    g.seq0.name = "N/A"; g.seq0.comment = "";   // printRepDBClusterResult's text for genomes without record infos (src/sub_command.cpp:688-693)
    st.genomes.push_back(g);
  }
  ok = ok && rd(fp, index_size);
  for (size_t i = 0; ok && i < index_size; i++) {
    uint64_t h = 0; size_t ls = 0;
    ok = rd(fp, h) && rd(fp, ls) && ls < ((size_t)1 << 31) && skip_bytes(fp, ls * sizeof(int));
  }
  fclose(fp);
  if (!ok) { std::cerr << "ERROR: truncated or malformed RepDB: " << path << std::endl; return false; }
  if (st.clusters.size() != rep_count) { std::cerr << "ERROR: " << st.clusters.size() << " clusters for " << rep_count << " representatives" << std::endl; return false; }
  std::cerr << "MinHash RepDB loaded from: " << path << std::endl
            << "  Representatives: " << rep_count << std::endl
            << "  Total genomes:   " << all_count << std::endl
            << "  Inverted index:  " << index_size << " unique hashes" << std::endl
            << "  Threshold:       " << st.threshold << std::endl
            << "  Kmer size:       " << st.kmer_size << std::endl
            << "  Sketch size:     " << st.sketch_size << std::endl
            << "  Containment:     " << (st.is_containment ? "yes" : "no") << std::endl;
  return true;
}

// src/greedy.cpp:2656-2765
void print_kssd_repdb_stats(const KssdClusterState& st, std::ostream& out) {
  size_t total_genomes = 0;
  for (const auto& cl : st.clusters) total_genomes += cl.size();
  const size_t nrep = st.rep_ids.size();
  auto rep_size = [&](size_t r) { return st.reps.use64 ? st.reps.h64[r].size() : st.reps.h32[r].size(); };
  out << "========================================" << std::endl;
  out << (st.minhash ? "    MinHash RepDB Statistics Report" : "        RepDB Statistics Report") << std::endl;
  out << "========================================" << std::endl << std::endl;
  out << "[Basic Info]" << std::endl;
  out << "  Threshold:              " << st.threshold << std::endl;
  out << "  Kmer size:              " << st.kmer_size << std::endl;
  if (st.minhash) {
    out << "  Sketch size:            " << st.sketch_size << std::endl;
    out << "  Containment mode:       " << (st.is_containment ? "yes" : "no") << std::endl << std::endl;
  } else {
    out << "  KSSD half_k:            " << st.info.half_k << std::endl;
    out << "  KSSD half_subk:         " << st.info.half_subk << std::endl;
    out << "  KSSD drlevel:           " << st.info.drlevel << std::endl << std::endl;
  }
  out << "[Scale]" << std::endl;
  out << "  Total genomes:          " << total_genomes << std::endl;
  out << "  Representatives:        " << nrep << std::endl;
  out << "  Clusters:               " << st.clusters.size() << std::endl;
  const double compression = total_genomes > 0 ? (1.0 - (double)nrep / total_genomes) * 100.0 : 0.0;
  out << "  Compression ratio:      " << std::fixed << std::setprecision(2) << compression << "%" << std::endl << std::endl;
  // the inverted index, from the representatives' sketches
  std::vector<uint64_t> keys;
  for (size_t r = 0; r < nrep; r++) {
    if (st.reps.use64) keys.insert(keys.end(), st.reps.h64[r].begin(), st.reps.h64[r].end());
    else keys.insert(keys.end(), st.reps.h32[r].begin(), st.reps.h32[r].end());
  }
  std::sort(keys.begin(), keys.end());
  size_t unique = 0, max_posting = 0;
  for (size_t i = 0; i < keys.size();) {
    size_t j = i;
    while (j < keys.size() && keys[j] == keys[i]) j++;
    unique++; max_posting = std::max(max_posting, j - i);
    i = j;
  }
  out << "[Inverted Index]" << std::endl;
  out << "  Unique hashes:          " << unique << std::endl;
  out << "  Total postings:         " << keys.size() << std::endl;
  out << "  Avg posting length:     " << std::fixed << std::setprecision(2) << (unique ? (double)keys.size() / unique : 0.0) << std::endl;
  out << "  Max posting length:     " << max_posting << std::endl << std::endl;
  out << "[Cluster Size Distribution]" << std::endl;
  if (!st.clusters.empty()) {
    std::vector<int> sizes;
    size_t singleton = 0;
    for (const auto& cl : st.clusters) { sizes.push_back((int)cl.size()); if (cl.size() <= 1) singleton++; }
    std::sort(sizes.begin(), sizes.end());
    out << "  Min cluster size:       " << sizes.front() << std::endl;
    out << "  Max cluster size:       " << sizes.back() << std::endl;
    out << "  Mean cluster size:      " << std::fixed << std::setprecision(2) << (double)total_genomes / st.clusters.size() << std::endl;
    out << "  Median cluster size:    " << sizes[sizes.size() / 2] << std::endl;
    out << "  Singletons:             " << singleton << " (" << std::fixed << std::setprecision(1)
        << (100.0 * singleton / st.clusters.size()) << "%)" << std::endl;
    out << "  P90 cluster size:       " << sizes[(size_t)(sizes.size() * 0.9)] << std::endl;
    out << "  P95 cluster size:       " << sizes[(size_t)(sizes.size() * 0.95)] << std::endl;
    out << "  P99 cluster size:       " << sizes[(size_t)(sizes.size() * 0.99)] << std::endl;
  }
  if (!st.minhash) out << std::endl << "[Representative Sketch Sizes]" << std::endl;   // (the MinHash report has no such section)
  if (nrep && !st.minhash) {
    size_t min_sk = SIZE_MAX, max_sk = 0, sum_sk = 0;
    for (size_t r = 0; r < nrep; r++) { const size_t z = rep_size(r); min_sk = std::min(min_sk, z); max_sk = std::max(max_sk, z); sum_sk += z; }
    out << "  Min sketch size:        " << min_sk << std::endl;
    out << "  Max sketch size:        " << max_sk << std::endl;
    out << "  Mean sketch size:       " << std::fixed << std::setprecision(1) << (double)sum_sk / nrep << std::endl;
  }
  uint64_t total_seq_len = 0, rep_seq_len = 0;
  for (const GenomeInfo& g : st.genomes) total_seq_len += g.totalSeqLength;
  if (total_seq_len > 0) {
    for (const GenomeInfo& g : st.rep_genomes) rep_seq_len += g.totalSeqLength;
    out << std::endl << "[Genome Coverage]" << std::endl;
    out << "  Total sequence length:  " << total_seq_len << " bp" << std::endl;
    out << "  Representative seq len: " << rep_seq_len << " bp" << std::endl;
    out << "  Coverage ratio:         " << std::fixed << std::setprecision(2) << (100.0 * rep_seq_len / total_seq_len) << "%" << std::endl;
  }
  out << "========================================" << std::endl;
}

void print_result(const std::vector<std::vector<int>>& cluster, const std::vector<GenomeInfo>& g, bool sketchByFile,
                  const std::string& outputFile, double threshold) {
  FILE* fp = fopen(outputFile.c_str(), "w");
  if (!fp) { std::cerr << "Error in printResult(), cannot open file: " << outputFile << std::endl; exit(1); }
  if (threshold >= 0.0) {
    fprintf(fp, "# Clustering threshold: %.6f\n", threshold);
    fprintf(fp, "# Total clusters: %zu\n", cluster.size());
    fprintf(fp, "#\n");
  }
  for (size_t i = 0; i < cluster.size(); i++) {
    fprintf(fp, "the cluster %d is: \n", (int)i);
    for (size_t j = 0; j < cluster[i].size(); j++) {
      const int curId = cluster[i][j];
      if (curId < 0 || curId >= (int)g.size()) continue;
      const GenomeInfo& s = g[curId];
      if (sketchByFile)
        fprintf(fp, "\t%5d\t%6d\t%12dnt\t%20s\t%20s\t%s\n", (int)j, curId, (int)s.totalSeqLength, s.fileName.c_str(),
                s.seq0.name.c_str(), s.seq0.comment.c_str());
      else
        fprintf(fp, "\t%6d\t%6d\t%12dnt\t%20s\t%s\n", (int)j, curId, s.seq0.length, s.seq0.name.c_str(), s.seq0.comment.c_str());
    }
    fprintf(fp, "\n");
  }
  fclose(fp);
}

// ---- --auto-threshold / --stability (src/MST.cpp:1743-2376) ----
EdgeLengthStats edge_length_stats(const std::vector<rtc_edge>& mst) {  // analyzeEdgeLengthDistribution, :1742-1816
  EdgeLengthStats s;
  for (const rtc_edge& e : mst) if (e.dist > 1e-10) s.sorted_distances.push_back(e.dist);  // zero edges (identical genomes) left out
  std::vector<double>& d = s.sorted_distances;
  std::sort(d.begin(), d.end());
  const int n = (int)d.size();
  if (n == 0) return s;
  s.min_dist = d[0];
  s.max_dist = d[n - 1];
  if (n == 1) { s.median_dist = s.mean_dist = s.q1_dist = s.q3_dist = d[0]; return s; }
  s.median_dist = n % 2 == 0 ? (d[n / 2 - 1] + d[n / 2]) / 2.0 : d[n / 2];
  s.q1_dist = d[std::max(0, n / 4)];
  s.q3_dist = d[std::min(n - 1, 3 * n / 4)];
  double sum = 0.0;
  for (double x : d) sum += x;
  s.mean_dist = sum / n;
  double var = 0.0;
  for (double x : d) { const double dx = x - s.mean_dist; var += dx * dx; }
  s.std_dev = sqrt(var / n);
  return s;
}

StabilityResult threshold_stability(const std::vector<rtc_edge>& mst, double threshold, int num_vertices, double epsilon,
                                    int num_samples, int min_near_edges) {  // computeThresholdStability, :1827-1955
  StabilityResult r;
  if (num_vertices <= 0 || mst.empty()) return r;
  // the window [threshold - eps, threshold + eps] grows by 1.5x until it holds min_near_edges edges or eps passes threshold / 2
  double lo = std::max(0.0, threshold - epsilon), hi = threshold + epsilon;
  const double eps_max = threshold * 0.5;
  std::vector<double> near;
  for (double eps = epsilon; near.size() < (size_t)min_near_edges && eps <= eps_max;) {
    lo = std::max(0.0, threshold - eps);
    hi = threshold + eps;
    near.clear();
    for (const rtc_edge& e : mst) if (e.dist >= lo && e.dist <= hi) near.push_back(e.dist);
    if (near.size() < (size_t)min_near_edges) eps *= 1.5;
  }
  r.near_edge_count = (int)near.size();
  if (near.empty()) { r.overall = r.split = r.merge = 1.0; return r; }
  std::sort(near.begin(), near.end());
  const double step = num_samples > 1 ? (hi - lo) / (num_samples - 1) : 0.0;
  double all = 0.0, split = 0.0, merge = 0.0;
  int n_all = 0, n_split = 0, n_merge = 0;
  for (int k = 0; k < num_samples; k++) {
    const double t = lo + k * step;
    if (t < 0.0) continue;
    // consistency = share of the near edges that stay on their side: those in (min(t, threshold), max(t, threshold)] flip
    double c = 1.0;
    if (!(fabs(t - threshold) < 1e-10)) {
      const auto a = std::upper_bound(near.begin(), near.end(), std::min(threshold, t));
      const auto b = std::upper_bound(near.begin(), near.end(), std::max(threshold, t));
      c = (double)((int)near.size() - (int)(b - a)) / near.size();
    }
    all += c; n_all++;
    if (t < threshold) { split += c; n_split++; }
    else if (t > threshold) { merge += c; n_merge++; }
  }
  if (n_all > 0) r.overall = all / n_all;
  if (n_split > 0) r.split = split / n_split;
  if (n_merge > 0) r.merge = merge / n_merge;
  r.overall = std::min(r.split, r.merge);
  return r;
}

namespace {
const char* gap_level(double t) {  // :2063-2077 (and the percentile candidates, :2137-2151)
  return t < 0.001 ? "identical/near-identical" : t < 0.005 ? "strain/subspecies" : t < 0.01 ? "strain" : t < 0.03 ? "species"
       : t < 0.1 ? "genus" : t < 0.2 ? "family" : "higher";
}
// the stability fields and the cluster count of a candidate (:2088-2105): cluster count whenever the vertex count is known
void fill_candidate(ThresholdCandidate& c, const std::vector<rtc_edge>& mst, bool enable_stability, int num_vertices) {
  if (num_vertices <= 0) return;
  if (enable_stability) {
    const StabilityResult s = threshold_stability(mst, c.threshold, num_vertices, 0.01, 5, 100);
    c.stability_score = s.overall; c.stability_split = s.split; c.stability_merge = s.merge; c.near_edge_count = s.near_edge_count;
  }
  c.cluster_count = (int)generate_cluster_with_bfs(generate_forest(mst, c.threshold), num_vertices).size();
}
}  // namespace

std::vector<ThresholdCandidate> threshold_candidates(const std::vector<rtc_edge>& mst, int max_candidates, double min_gap_ratio,
                                                     bool enable_stability, int num_vertices) {  // findThresholdCandidates, :1957-2178
  std::vector<ThresholdCandidate> out;
  if (mst.size() < 2) return out;
  const EdgeLengthStats st = edge_length_stats(mst);
  const std::vector<double>& d = st.sorted_distances;
  const int n = (int)d.size();
  const double range = st.max_dist - st.min_dist;
  if (range <= 1e-10) {  // one distance only: the median, with the coarser level scale of :1990-1998
    ThresholdCandidate c;
    c.threshold = st.median_dist;
    c.confidence = 0.5;
    c.level = c.threshold < 0.01 ? "strain" : c.threshold < 0.03 ? "species" : c.threshold < 0.1 ? "genus" : "higher";
    fill_candidate(c, mst, enable_stability, num_vertices);
    out.push_back(c);
    return out;
  }
  const double min_gap = range * min_gap_ratio;
  std::vector<std::pair<double, int>> gaps;  // (gap, index of the larger distance)
  for (int i = 1; i < n; i++) {
    const double gap = d[i] - d[i - 1];
    if (gap > min_gap) gaps.push_back({gap, i});
  }
  // largest first; equal gaps in the order std::sort leaves them, as in the reference (:2040-2043)
  std::sort(gaps.begin(), gaps.end(), [](const std::pair<double, int>& a, const std::pair<double, int>& b) { return a.first > b.first; });
  for (int i = 0; i < std::min(max_candidates, (int)gaps.size()); i++) {
    ThresholdCandidate c;
    c.edge_index = gaps[i].second;
    c.threshold = d[c.edge_index];
    c.gap_score = gaps[i].first;
    c.confidence = std::min(1.0, gaps[i].first / range * 10.0);
    c.level = gap_level(c.threshold);
    fill_candidate(c, mst, enable_stability, num_vertices);
    out.push_back(c);
  }
  // Q1 (unless below 0.001), median and Q3 where they lie strictly inside the range and not within min_gap / 2 of a candidate
  std::vector<double> pct;
  if (st.q1_dist >= 0.001) pct.push_back(st.q1_dist);
  pct.push_back(st.median_dist);
  pct.push_back(st.q3_dist);
  for (double t : pct) {
    if (t < 0.001) continue;
    bool close = false;
    for (const ThresholdCandidate& c : out) if (fabs(c.threshold - t) < min_gap * 0.5) { close = true; break; }
    if (close || !(t > st.min_dist && t < st.max_dist)) continue;
    ThresholdCandidate c;
    c.threshold = t;
    c.confidence = 0.4;
    c.level = gap_level(t);
    fill_candidate(c, mst, enable_stability, num_vertices);
    out.push_back(c);
  }
  std::sort(out.begin(), out.end(), [](const ThresholdCandidate& a, const ThresholdCandidate& b) { return a.threshold < b.threshold; });
  return out;
}

// selectOptimalThreshold, :2180-2269.  Where the reference leaves fields of its result uninitialised (the empty list, the
// fallback when no candidate reaches 0.001) they hold ThresholdCandidate's defaults here: no gap, edge index -1, stability
// 0.5, no cluster count.
ThresholdCandidate select_optimal_threshold(const std::vector<ThresholdCandidate>& candidates, const std::vector<rtc_edge>& mst) {
  ThresholdCandidate opt;
  if (candidates.empty()) { opt.threshold = 0.05; opt.confidence = 0.0; opt.level = "unknown"; return opt; }
  double best = -1.0;
  bool in_range = false;
  for (const ThresholdCandidate& c : candidates) {
    if (c.threshold < 0.001) continue;
    double score = c.confidence;
    if (c.threshold >= 0.01 && c.threshold <= 0.1) { score *= 2.0; in_range = true; }
    else if (c.threshold >= 0.001 && c.threshold < 0.01) score *= 1.2;
    else if (c.threshold > 0.1 && c.threshold <= 0.2) score *= 1.1;
    if (c.gap_score > 0.0) score += c.gap_score * 20.0;
    if (score > best) { best = score; opt = c; }
  }
  if (!in_range && best < 0) {
    const double med = edge_length_stats(mst).median_dist;
    if (med >= 0.01 && med <= 0.2) {
      opt.threshold = med; opt.confidence = 0.4;
      opt.level = med < 0.03 ? "species" : med < 0.1 ? "genus" : "family";
    } else {
      opt.threshold = 0.05; opt.confidence = 0.3; opt.level = "genus";
    }
    opt.gap_score = 0.0; opt.edge_index = -1;
  }
  return opt;
}

void print_threshold_analysis(const std::vector<rtc_edge>& mst, const EdgeLengthStats& st, const std::vector<ThresholdCandidate>& cands,
                              const ThresholdCandidate& opt, const std::string& file) {  // printThresholdAnalysis, :2271-2376
  FILE* fp = fopen(file.c_str(), "w");
  if (!fp) { std::cerr << "ERROR: printThresholdAnalysis(), cannot write file: " << file << std::endl; return; }
  fprintf(fp, "# Automatic Threshold Selection Analysis\n# Based on MST Edge Length Distribution\n# ===========================================\n\n");
  fprintf(fp, "## Edge Length Statistics\n");
  fprintf(fp, "Total edges: %zu\n", mst.size());
  fprintf(fp, "Min distance: %.6f\n", st.min_dist);
  fprintf(fp, "Max distance: %.6f\n", st.max_dist);
  fprintf(fp, "Mean distance: %.6f\n", st.mean_dist);
  fprintf(fp, "Median distance: %.6f\n", st.median_dist);
  fprintf(fp, "Q1 (25%%): %.6f\n", st.q1_dist);
  fprintf(fp, "Q3 (75%%): %.6f\n", st.q3_dist);
  fprintf(fp, "Standard deviation: %.6f\n", st.std_dev);
  fprintf(fp, "Range: %.6f\n\n", st.max_dist - st.min_dist);
  fprintf(fp, "## Optimal Threshold (Recommended)\n");
  fprintf(fp, "Threshold: %.6f\n", opt.threshold);
  fprintf(fp, "Confidence: %.3f\n", opt.confidence);
  if (opt.cluster_count > 0 || opt.stability_score != 0.5) {
    fprintf(fp, "Stability (overall): %.3f\n", opt.stability_score);
    if (opt.stability_split != 0.5 || opt.stability_merge != 0.5) {
      fprintf(fp, "  - Split sensitivity: %.3f (stability when threshold decreases)\n", opt.stability_split);
      fprintf(fp, "  - Merge sensitivity: %.3f (stability when threshold increases)\n", opt.stability_merge);
    }
    if (opt.near_edge_count > 0) fprintf(fp, "  - Near edges evaluated: %d\n", opt.near_edge_count);
    fprintf(fp, "Number of clusters: %d\n", opt.cluster_count);
  }
  fprintf(fp, "Suggested level: %s\n", opt.level.c_str());
  if (opt.edge_index >= 0) {
    fprintf(fp, "Edge index: %d\nGap score: %.6f\n", opt.edge_index, opt.gap_score);
    fprintf(fp, "Source: gap-based detection (natural breakpoint in edge distribution)\n");
  } else {
    fprintf(fp, "Source: percentile-based (median/quartile, no significant gap detected)\n");
    fprintf(fp, "Note: This threshold is based on distribution statistics, not natural breakpoints.\n");
    fprintf(fp, "      Consider manual adjustment (e.g., 0.01-0.05 for species/genus level) if needed.\n");
  }
  fprintf(fp, "\n## All Candidate Thresholds\n");
  bool wide = false;  // stability columns once any candidate carries a cluster count or a stability score
  for (const ThresholdCandidate& c : cands) if (c.cluster_count > 0 || c.stability_score != 0.5) { wide = true; break; }
  if (wide) {
    fprintf(fp, "# Threshold\tConfidence\tStability_Overall\tStability_Split\tStability_Merge\tNear_Edges\tClusters\tLevel\tGap_Score\tEdge_Index\n");
    for (const ThresholdCandidate& c : cands)
      fprintf(fp, "%.6f\t%.3f\t%.3f\t%.3f\t%.3f\t%d\t%d\t%s\t%.6f\t%d\n", c.threshold, c.confidence, c.stability_score, c.stability_split,
              c.stability_merge, c.near_edge_count, c.cluster_count, c.level.c_str(), c.gap_score, c.edge_index);
  } else {
    fprintf(fp, "# Threshold\tConfidence\tLevel\tGap_Score\tEdge_Index\n");
    for (const ThresholdCandidate& c : cands)
      fprintf(fp, "%.6f\t%.3f\t%s\t%.6f\t%d\n", c.threshold, c.confidence, c.level.c_str(), c.gap_score, c.edge_index);
  }
  fprintf(fp, "\n## Edge Length Distribution (sorted)\n# Index\tDistance\n");
  for (size_t i = 0; i < st.sorted_distances.size(); i++) fprintf(fp, "%zu\t%.6f\n", i, st.sorted_distances[i]);
  fclose(fp);
  std::cerr << "-----write threshold analysis into: " << file << std::endl;
}

// src/sub_command.cpp:1852-1879 (clust_from_mst), :2032-2059 (compute_kssd_clusters), :2549-2566 / :2786-2803 (--presketched)
void auto_threshold_report(const std::vector<rtc_edge>& mst, int num_vertices, const std::string& outputFile, double min_gap_ratio,
                           bool stability) {
  if (mst.empty()) { std::cerr << "-----WARNING: MST is empty, cannot perform automatic threshold selection" << std::endl; return; }
  if (mst.size() < 2) {
    std::cerr << "-----WARNING: MST has only " << mst.size() << " edge(s), cannot perform automatic threshold selection" << std::endl;
    return;
  }
  std::cerr << "-----analyzing MST edge length distribution for automatic threshold selection..." << std::endl;
  if (stability) std::cerr << "-----stability evaluation enabled (this may take longer)..." << std::endl;
  const EdgeLengthStats st = edge_length_stats(mst);
  const std::vector<ThresholdCandidate> cands = threshold_candidates(mst, 5, min_gap_ratio, stability, num_vertices);
  const ThresholdCandidate opt = select_optimal_threshold(cands, mst);
  const std::string file = outputFile + ".threshold_analysis.txt";
  print_threshold_analysis(mst, st, cands, opt, file);
  std::cerr << "-----optimal threshold: " << opt.threshold << " (confidence: " << opt.confidence << ", suggested level: " << opt.level << ")"
            << std::endl;
  if (stability) {
    std::cerr << "-----stability: " << opt.stability_score << " (split: " << opt.stability_split << ", merge: " << opt.stability_merge << ")"
              << std::endl;
    std::cerr << "-----near edges: " << opt.near_edge_count << ", clusters: " << opt.cluster_count << std::endl;
  }
  std::cerr << "-----threshold analysis written to: " << file << std::endl;
}

// src/sub_command.cpp:1880-1892, :2060-2072: --stability without --auto-threshold, at the user's threshold
void stability_report(const std::vector<rtc_edge>& mst, int num_vertices, double threshold) {
  if (mst.empty()) { std::cerr << "-----WARNING: MST is empty, cannot evaluate threshold stability" << std::endl; return; }
  std::cerr << "-----evaluating stability for threshold: " << threshold << "..." << std::endl;
  const StabilityResult s = threshold_stability(mst, threshold, num_vertices, 0.01, 5, 100);
  const size_t nc = generate_cluster_with_bfs(generate_forest(mst, threshold), num_vertices).size();
  std::cerr << "-----threshold stability: " << s.overall << " (split: " << s.split << ", merge: " << s.merge << ")" << std::endl;
  std::cerr << "-----near edges evaluated: " << s.near_edge_count << ", clusters: " << nc << std::endl;
}

// ---- --dedup-dist / --reps-per-cluster (src/cluster_postprocess.cpp) ----
bool tree_medoids_host(int n, const std::vector<rtc_edge>& forest, double dedup_dist, const std::vector<uint64_t>& seq_len,
                       std::vector<int>& node_to_rep, int threads) {
  node_to_rep.resize(n);
  if (!(dedup_dist > 0)) { for (int i = 0; i < n; i++) node_to_rep[i] = i; return true; }
  rtc_tm::Groups G;
  if (!rtc_tm::build_groups(n, forest.data(), forest.size(), dedup_dist, G)) return false;
  std::vector<uint32_t> all(G.count());
  for (size_t g = 0; g < all.size(); g++) all[g] = (uint32_t)g;
  std::vector<double> tot(G.mem.size());
  rtc_tm::totals_host(G, all, tot.data(), threads);
  rtc_tm::assign(G, n, tot.data(), seq_len.empty() ? nullptr : seq_len.data(), node_to_rep.data());
  return true;
}

std::vector<std::vector<int>> dedup_candidates(const std::vector<std::vector<int>>& clusters, const std::vector<int>& node_to_rep,
                                               double dedup_dist) {
  if (!(dedup_dist > 0)) return clusters;
  const int n = (int)node_to_rep.size();
  std::vector<std::vector<int>> out;
  out.reserve(clusters.size());
  for (const std::vector<int>& cl : clusters) {
    std::vector<int> c;
    for (int v : cl) {
      if (v < 0 || v >= n) continue;
      c.push_back(node_to_rep[v] < 0 ? v : node_to_rep[v]);
    }
    std::sort(c.begin(), c.end());
    c.erase(std::unique(c.begin(), c.end()), c.end());
    out.push_back(std::move(c));
  }
  return out;
}

namespace {
// tree distances from `s` over a component's local adjacency (-1: not reached); the stack walk of distances_from, :33-54
void tree_dist(int s, const std::vector<std::vector<std::pair<int, double>>>& adj, std::vector<double>& dist, std::vector<int>& parent,
               std::vector<int>& stack) {
  dist.assign(adj.size(), -1.0);
  parent.assign(adj.size(), -1);
  stack.clear();
  dist[s] = 0.0; parent[s] = s;
  stack.push_back(s);
  while (!stack.empty()) {
    const int u = stack.back();
    stack.pop_back();
    for (const auto& vw : adj[u]) {
      if (vw.first == parent[u]) continue;
      parent[vw.first] = u;
      dist[vw.first] = dist[u] + vw.second;
      stack.push_back(vw.first);
    }
  }
}
}  // namespace

std::vector<std::vector<int>> select_k_reps(const std::vector<std::vector<int>>& clusters, const std::vector<std::vector<int>>& candidates,
                                            const std::vector<rtc_edge>& forest, int n, const std::vector<int>& node_to_rep, int k) {
  std::vector<std::vector<int>> reps(clusters.size());
  if (k <= 0) return reps;
  std::vector<std::vector<std::pair<int, double>>> adj(n);
  for (const rtc_edge& e : forest) {
    if (e.preNode < 0 || e.preNode >= n || e.sufNode < 0 || e.sufNode >= n) continue;
    adj[e.preNode].push_back({e.sufNode, e.dist});
    adj[e.sufNode].push_back({e.preNode, e.dist});
  }
  std::vector<int> local(n, -1);  // node -> position in the current cluster
  std::vector<double> dist;
  std::vector<int> parent, stack;
  for (size_t ci = 0; ci < clusters.size(); ci++) {
    const std::vector<int>& comp = clusters[ci];
    const std::vector<int>& cand = candidates[ci];
    if (cand.empty()) continue;
    if ((int)cand.size() <= k) { reps[ci] = cand; continue; }
    const int m = (int)comp.size();
    for (int i = 0; i < m; i++) local[comp[i]] = i;
    std::vector<std::vector<std::pair<int, double>>> ladj(m);
    for (int i = 0; i < m; i++)
      for (const auto& vw : adj[comp[i]]) if (local[vw.first] >= 0) ladj[i].push_back({local[vw.first], vw.second});
    auto farthest = [&](int s) {  // first of the largest distances (:166-178)
      tree_dist(s, ladj, dist, parent, stack);
      int far = s; double best = -1.0;
      for (int i = 0; i < m; i++) if (dist[i] > best) { best = dist[i]; far = i; }
      return far;
    };
    const int u = farthest(0), v = farthest(u);  // the diameter's ends (:234-237)
    std::vector<int> cand_sorted(cand);
    std::sort(cand_sorted.begin(), cand_sorted.end());
    auto is_cand = [&](int x) { return std::binary_search(cand_sorted.begin(), cand_sorted.end(), x); };
    auto to_cand = [&](int node) {  // map_to_candidate, :244-249
      const int r = node >= 0 && node < (int)node_to_rep.size() ? node_to_rep[node] : node;
      if (is_cand(r)) return r;
      if (is_cand(node)) return node;
      return cand[0];
    };
    std::vector<int> chosen;
    auto taken = [&](int x) { return std::find(chosen.begin(), chosen.end(), x) != chosen.end(); };
    const int r1 = to_cand(comp[u]);
    chosen.push_back(r1);
    if ((int)chosen.size() < k) { const int r2 = to_cand(comp[v]); if (!taken(r2)) chosen.push_back(r2); }
    std::vector<double> min_dist(m, std::numeric_limits<double>::infinity());
    auto add = [&](int rep) {
      if (rep < 0 || rep >= n || local[rep] < 0) return;
      tree_dist(local[rep], ladj, dist, parent, stack);
      for (int i = 0; i < m; i++) if (dist[i] >= 0.0 && dist[i] < min_dist[i]) min_dist[i] = dist[i];
    };
    for (int r : chosen) add(r);
    std::vector<int> cand_local;
    for (int c : cand) if (c >= 0 && c < n && local[c] >= 0) cand_local.push_back(local[c]);
    while ((int)chosen.size() < k) {  // farthest-first: the candidate farthest from every chosen one (:280-298)
      int best_i = -1; double best = -1.0;
      for (int li : cand_local) {
        if (taken(to_cand(comp[li]))) continue;
        if (min_dist[li] > best) { best = min_dist[li]; best_i = li; }
      }
      if (best_i < 0) break;
      const int next = to_cand(comp[best_i]);
      if (taken(next)) break;
      chosen.push_back(next);
      add(next);
    }
    for (int i = 0; i < m; i++) local[comp[i]] = -1;
    std::sort(chosen.begin(), chosen.end());
    reps[ci] = std::move(chosen);
  }
  return reps;
}

// ---- clust-mst --save-rep / --append state (src/mst_state.cpp) ----
namespace {
template <typename T> void mw_pod(std::ofstream& o, const T& v) { o.write(reinterpret_cast<const char*>(&v), sizeof(T)); }
template <typename T> void mr_pod(std::ifstream& i, T& v) { i.read(reinterpret_cast<char*>(&v), sizeof(T)); }
void mw_str(std::ofstream& o, const std::string& s) {
  const uint32_t n = (uint32_t)s.size();
  mw_pod(o, n);
  if (n) o.write(s.data(), n);
}
bool mr_str(std::ifstream& i, std::string& s) {
  uint32_t n = 0;
  mr_pod(i, n);
  if (!i) return false;
  s.resize(n);
  if (n) i.read(&s[0], n);
  return (bool)i;
}
template <typename T> void mw_vec(std::ofstream& o, const std::vector<T>& v) {
  const uint64_t n = v.size();
  mw_pod(o, n);
  if (n) o.write(reinterpret_cast<const char*>(v.data()), sizeof(T) * n);
}
template <typename T> bool mr_vec(std::ifstream& i, std::vector<T>& v) {
  uint64_t n = 0;
  mr_pod(i, n);
  if (!i) return false;
  // a length past what is left of the file is a damaged file, not a request for memory
  const std::streampos here = i.tellg();
  i.seekg(0, std::ios::end);
  const std::streampos end = i.tellg();
  i.seekg(here);
  if (n > (uint64_t)(end - here) / sizeof(T)) { i.setstate(std::ios::failbit); return false; }
  v.resize(n);
  if (n) i.read(reinterpret_cast<char*>(v.data()), sizeof(T) * n);
  return (bool)i;
}
// build_inverted_index_from_reps: hash -> the representatives that hold it, ascending
template <typename T> std::vector<std::pair<T, std::vector<int>>> mst_index(const std::vector<std::vector<T>>& reps) {
  std::vector<std::pair<T, int>> all;
  for (size_t r = 0; r < reps.size(); r++) for (T h : reps[r]) all.push_back({h, (int)r});
  std::sort(all.begin(), all.end());
  std::vector<std::pair<T, std::vector<int>>> idx;
  for (size_t a = 0; a < all.size(); a++) {
    if (idx.empty() || idx.back().first != all[a].first) idx.push_back({all[a].first, {}});
    idx.back().second.push_back(all[a].second);
  }
  return idx;
}
template <typename T> void mw_index(std::ofstream& o, const std::vector<std::vector<T>>& reps, uint64_t& H) {
  const auto idx = mst_index(reps);
  H = idx.size();
  mw_pod(o, H);
  for (const auto& kv : idx) { mw_pod(o, kv.first); mw_vec(o, kv.second); }
}
template <typename T> bool mr_index(std::ifstream& i, uint64_t& H) {
  mr_pod(i, H);
  for (uint64_t a = 0; a < H && i; a++) { T h; std::vector<int> lst; mr_pod(i, h); if (!mr_vec(i, lst)) return false; }
  return (bool)i;
}
// UnionFind.h: path compression, union by rank (equal ranks: the second argument's root wins)
struct MstUF {
  std::vector<int> parent, rank;
  explicit MstUF(int n) : parent(n), rank(n, 0) { for (int i = 0; i < n; i++) parent[i] = i; }
  void extend() { parent.push_back((int)parent.size()); rank.push_back(0); }
  int find(int x) { while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; } return x; }
  void merge(int x, int y) {
    x = find(x); y = find(y);
    if (x == y) return;
    if (rank[x] > rank[y]) parent[y] = x;
    else if (rank[x] < rank[y]) parent[x] = y;
    else { parent[x] = y; rank[y]++; }
  }
};
}  // namespace

bool save_mst_state(const std::string& path, const MstState& st) {
  std::ofstream o(path, std::ios::binary);
  if (!o) { std::cerr << "ERROR: " << (st.kssd ? "KssdMstState" : "MinHashMstState") << "::save cannot open " << path << std::endl; return false; }
  o.write(st.kssd ? "KSMSTST01" : "MHMSTST01", 9);
  mw_pod(o, st.threshold);
  mw_pod(o, st.kmer_size);
  if (st.kssd) { mw_pod(o, st.half_k); mw_pod(o, st.half_subk); mw_pod(o, st.drlevel); mw_pod(o, st.use64); }
  else { mw_pod(o, st.sketch_size); mw_pod(o, st.contain_compress); mw_pod(o, st.is_containment); }
  mw_pod(o, st.sketch_by_file);
  mw_pod(o, st.N);
  const uint64_t R = st.reps();
  mw_pod(o, R);
  for (uint64_t r = 0; r < R; r++) {
    const int rid = r < st.rep_ids.size() ? st.rep_ids[r] : -1;
    mw_pod(o, rid);
    const uint64_t tlen = r < st.rep_lens.size() ? st.rep_lens[r] : 0;
    mw_pod(o, tlen);
    mw_str(o, r < st.rep_names.size() ? st.rep_names[r] : std::string());
    if (st.use64) mw_vec(o, st.h64[r]);
    else mw_vec(o, st.h32[r]);
  }
  const uint64_t C = st.clusters.size();
  mw_pod(o, C);
  for (const auto& cl : st.clusters) mw_vec(o, cl);
  const uint64_t M = st.member_names.size();
  mw_pod(o, M);
  for (const auto& nm : st.member_names) mw_str(o, nm);
  mw_vec(o, st.member_lens);
  uint64_t H = 0;
  if (st.use64) mw_index(o, st.h64, H);
  else mw_index(o, st.h32, H);
  o.close();
  if (st.kssd)
    std::cerr << "Saved KSSD MST state to " << path << " (reps=" << R << ", clusters=" << C << ", members=" << M << ")" << std::endl;
  else
    std::cerr << "Saved MinHash MST state to " << path << " (reps=" << R << ", clusters=" << C << ", members=" << M
              << ", unique_hashes=" << H << ")" << std::endl;
  return (bool)o;
}

bool load_mst_state(const std::string& path, bool kssd, MstState& st) {
  const char* who = kssd ? "KssdMstState" : "MinHashMstState";
  std::ifstream i(path, std::ios::binary);
  if (!i) { std::cerr << "ERROR: " << who << "::load cannot open " << path << std::endl; return false; }
  char magic[10] = {0};
  i.read(magic, 9);
  if (memcmp(magic, kssd ? "KSMSTST01" : "MHMSTST01", 9) != 0) {
    std::cerr << "ERROR: " << path << " is not a " << (kssd ? "KSSD" : "MinHash") << " MST state (bad magic)" << std::endl;
    return false;
  }
  st = MstState();
  st.kssd = kssd;
  mr_pod(i, st.threshold);
  mr_pod(i, st.kmer_size);
  if (kssd) { mr_pod(i, st.half_k); mr_pod(i, st.half_subk); mr_pod(i, st.drlevel); mr_pod(i, st.use64); }
  else { mr_pod(i, st.sketch_size); mr_pod(i, st.contain_compress); mr_pod(i, st.is_containment); st.use64 = true; }
  mr_pod(i, st.sketch_by_file);
  mr_pod(i, st.N);
  uint64_t R = 0, C = 0, M = 0, H = 0;
  mr_pod(i, R);
  bool ok = (bool)i && R <= (uint64_t)INT32_MAX;
  for (uint64_t r = 0; ok && r < R; r++) {
    int rid = 0; uint64_t tlen = 0; std::string nm;
    mr_pod(i, rid); mr_pod(i, tlen);
    ok = mr_str(i, nm);
    st.rep_ids.push_back(rid); st.rep_lens.push_back(tlen); st.rep_names.push_back(nm);
    if (st.use64) { st.h64.emplace_back(); ok = ok && mr_vec(i, st.h64.back()); }
    else { st.h32.emplace_back(); ok = ok && mr_vec(i, st.h32.back()); }
  }
  if (ok) { mr_pod(i, C); ok = (bool)i && C <= (uint64_t)INT32_MAX; }
  for (uint64_t c = 0; ok && c < C; c++) { st.clusters.emplace_back(); ok = mr_vec(i, st.clusters.back()); }
  if (ok) { mr_pod(i, M); ok = (bool)i && M <= (uint64_t)INT32_MAX; }
  for (uint64_t m = 0; ok && m < M; m++) { st.member_names.emplace_back(); ok = mr_str(i, st.member_names.back()); }
  ok = ok && mr_vec(i, st.member_lens);
  ok = ok && (st.use64 ? mr_index<uint64_t>(i, H) : mr_index<uint32_t>(i, H));
  if (!ok || st.clusters.size() != R) {
    std::cerr << "ERROR: " << path << " ends early or does not hold one cluster per representative" << std::endl;
    return false;
  }
  if (kssd)
    std::cerr << "Loaded KSSD MST state from " << path << " (reps=" << R << ", clusters=" << C << ", members=" << M << ")" << std::endl;
  else
    std::cerr << "Loaded MinHash MST state from " << path << " (reps=" << R << ", clusters=" << C << ", members=" << M
              << ", unique_hashes=" << H << ")" << std::endl;
  return true;
}

void init_mst_state(MstState& st, const std::vector<GenomeInfo>& g, bool sketchByFile, const std::vector<std::vector<int>>& clusters,
                    const std::vector<int>& rep_of_cluster, const std::vector<std::vector<uint64_t>>* h64,
                    const std::vector<std::vector<uint32_t>>* h32) {
  st.N = (int)g.size();
  st.sketch_by_file = sketchByFile;
  st.use64 = h64 != nullptr;
  auto len_of = [&](int id) { return sketchByFile ? g[id].totalSeqLength : (uint64_t)g[id].seq0.length; };
  for (int i = 0; i < st.N; i++) { st.member_names.push_back(g[i].fileName); st.member_lens.push_back(len_of(i)); }
  for (size_t c = 0; c < clusters.size(); c++) {
    if (clusters[c].empty()) continue;
    int rep = rep_of_cluster[c];
    if (rep < 0 || rep >= st.N) rep = clusters[c][0];
    st.rep_ids.push_back(rep);
    st.rep_names.push_back(g[rep].fileName);
    st.rep_lens.push_back(len_of(rep));
    if (h64) st.h64.push_back((*h64)[rep]);
    else st.h32.push_back((*h32)[rep]);
    st.clusters.push_back(clusters[c]);
  }
}

std::vector<std::vector<int>> append_mst_state(MstState& st, const std::vector<std::string>& names, const std::vector<uint64_t>& lens,
                                               const std::vector<std::vector<uint64_t>>* qh64, const std::vector<std::vector<uint32_t>>* qh32,
                                               const std::vector<rtc_rep_pair>& pairs) {
  const int R0 = (int)st.reps();
  const int Q = (int)names.size();
  MstUF uf(R0);
  std::vector<int> became(Q, -1);  // query -> its representative index, if it opened a cluster
  int assigned = 0, merges = 0, opened = 0;
  size_t p = 0;
  std::vector<std::pair<int, double>> matches;
  for (int q = 0; q < Q; q++) {
    matches.clear();
    for (; p < pairs.size() && (int)pairs[p].query == q; p++) {
      const int s = (int)pairs[p].slot;
      const int r = s < R0 ? s : became[s - R0];
      if (r < 0 || uf.find(r) != r) continue;  // not a representative, or merged away: its root's own count decides
      matches.push_back({r, pairs[p].dist});
    }
    const int id = st.N++;
    st.member_names.push_back(names[q]);
    st.member_lens.push_back(lens[q]);
    if (matches.empty()) {
      became[q] = (int)st.reps();
      st.rep_ids.push_back(id);
      st.rep_names.push_back(names[q]);
      st.rep_lens.push_back(lens[q]);
      if (st.use64) st.h64.push_back((*qh64)[q]);
      else st.h32.push_back((*qh32)[q]);
      st.clusters.push_back({id});
      uf.extend();
      opened++;
      continue;
    }
    size_t best = 0;  // decide_assignment: the closest; equal distances to the lowest slot (matches ascend by slot)
    for (size_t m = 1; m < matches.size(); m++) if (matches[m].second < matches[best].second) best = m;
    const int survivor = matches[best].first;
    for (size_t m = 0; m < matches.size(); m++) {
      if (m == best) continue;
      const int other_root = uf.find(matches[m].first), surv_root = uf.find(survivor);
      if (other_root == surv_root) continue;
      uf.merge(surv_root, other_root);
      const int new_root = uf.find(surv_root);
      const int loser = new_root == surv_root ? other_root : surv_root;
      auto& src = st.clusters[loser];
      auto& dst = st.clusters[new_root];
      dst.insert(dst.end(), src.begin(), src.end());
      src.clear();
      merges++;
    }
    st.clusters[uf.find(survivor)].push_back(id);
    assigned++;
  }
  std::cerr << "\n[clust-mst" << (st.kssd ? " --fast" : "") << " append summary]" << std::endl
            << "  assigned to existing : " << assigned << std::endl
            << "  new clusters         : " << opened << std::endl
            << "  cluster merges       : " << merges << std::endl;
  // collect_live_clusters + compact_*_state: the non-empty roots, in representative order
  std::vector<std::vector<int>> live;
  MstState out = st;
  out.rep_ids.clear(); out.rep_names.clear(); out.rep_lens.clear(); out.h64.clear(); out.h32.clear(); out.clusters.clear();
  for (int r = 0; r < (int)st.reps(); r++) {
    if (st.clusters[r].empty() || uf.find(r) != r) continue;
    live.push_back(st.clusters[r]);
    out.rep_ids.push_back(st.rep_ids[r]);
    out.rep_names.push_back(st.rep_names[r]);
    out.rep_lens.push_back(st.rep_lens[r]);
    if (st.use64) out.h64.push_back(std::move(st.h64[r]));
    else out.h32.push_back(std::move(st.h32[r]));
    out.clusters.push_back(std::move(st.clusters[r]));
  }
  st = std::move(out);
  return live;
}

// print_cluster_size_histogram + MinHashMstPrintStats / KssdMstPrintStats (src/mst_state.cpp:1342-1415)
void print_mst_state_stats(const MstState& st, std::ostream& os) {
  size_t uniq = 0;
  if (st.use64) {
    std::vector<uint64_t> all;
    for (const auto& h : st.h64) all.insert(all.end(), h.begin(), h.end());
    std::sort(all.begin(), all.end());
    uniq = (size_t)(std::unique(all.begin(), all.end()) - all.begin());
  } else {
    std::vector<uint32_t> all;
    for (const auto& h : st.h32) all.insert(all.end(), h.begin(), h.end());
    std::sort(all.begin(), all.end());
    uniq = (size_t)(std::unique(all.begin(), all.end()) - all.begin());
  }
  if (st.kssd) {
    os << "========== KSSD MST RepDB stats ==========\n";
    os << "  Kmer size:        " << st.kmer_size << "\n";
    os << "  half_k:           " << st.half_k << "\n";
    os << "  half_subk:        " << st.half_subk << "\n";
    os << "  drlevel:          " << st.drlevel << "\n";
    os << "  use64:            " << (st.use64 ? "yes" : "no") << "\n";
  } else {
    os << "========== MinHash MST RepDB stats ==========\n";
    os << "  Kmer size:        " << st.kmer_size << "\n";
    os << "  Sketch size:      " << st.sketch_size << "\n";
    os << "  Containment:      " << (st.is_containment ? "yes" : "no") << "\n";
    if (st.is_containment) os << "  Contain compress: " << st.contain_compress << "\n";
  }
  os << "  Threshold:        " << std::fixed << std::setprecision(6) << st.threshold << "\n";
  os << "  Total reps slots: " << st.reps() << "\n";
  os << "  sketch_by_file:   " << (st.sketch_by_file ? "yes" : "no") << "\n";
  os << "  Total members N:  " << st.N << "\n";
  if (!st.kssd) os << "  Inverted index:   " << uniq << " unique hashes\n";
  else os << "  Inverted index:   " << uniq << " unique hashes (" << (st.use64 ? "64" : "32") << "-bit)\n";
  int b1 = 0, b2 = 0, b3_5 = 0, b6_10 = 0, b11_100 = 0, b101_1000 = 0, bgt = 0, live = 0, total = 0, mx = 0;
  int mn = std::numeric_limits<int>::max();
  for (const auto& c : st.clusters) {
    const int sz = (int)c.size();
    if (sz == 0) continue;
    live++; total += sz;
    mx = std::max(mx, sz); mn = std::min(mn, sz);
    if (sz == 1) b1++;
    else if (sz == 2) b2++;
    else if (sz <= 5) b3_5++;
    else if (sz <= 10) b6_10++;
    else if (sz <= 100) b11_100++;
    else if (sz <= 1000) b101_1000++;
    else bgt++;
  }
  if (live == 0) mn = 0;
  os << "  Live clusters:    " << live << "\n";
  os << "  Total members:    " << total << "\n";
  os << "  Cluster size:     min=" << mn << " max=" << mx << " avg=" << std::fixed << std::setprecision(2)
     << (live ? (double)total / live : 0.0) << "\n";
  os << "  Size histogram:\n";
  os << "    size=1         : " << b1 << "\n";
  os << "    size=2         : " << b2 << "\n";
  os << "    size=3-5       : " << b3_5 << "\n";
  os << "    size=6-10      : " << b6_10 << "\n";
  os << "    size=11-100    : " << b11_100 << "\n";
  os << "    size=101-1000  : " << b101_1000 << "\n";
  os << "    size>1000      : " << bgt << "\n";
  os << (st.kssd ? "==========================================\n" : "==============================================\n");
}

std::vector<int> mst_live_index(const MstState& st) {
  std::vector<int> live(st.clusters.size(), -1);
  int n = 0;
  for (size_t i = 0; i < st.clusters.size(); i++) if (!st.clusters[i].empty()) live[i] = n++;
  return live;
}

int mst_query_wmode(const MstState& st) {
  if (st.kssd) return 0;
  if (st.is_containment) return 1;
  return 2 | (int)((uint32_t)std::max(st.sketch_size, 1) << 2);
}

double mst_query_distance(uint32_t common, uint32_t denom, int wmode, int kmer_size) {
  const double j = denom == 0 ? 0.0 : (double)common / (double)denom;
  double d;
  if ((wmode & 3) == 1) {  // containDistance
    if (j == 1.0) d = 0.0;
    else if (j == 0.0) d = 1.0;
    else d = -(1.0 / kmer_size) * log(j);
  } else {  // mash_distance (set Jaccard) / MinHash::distance (union-truncated Jaccard)
    if (j == 1.0) d = 0.0;
    else if (j == 0.0) d = 1.0;
    else { d = -log(2.0 * j / (1.0 + j)) / (double)kmer_size; if (d > 1.0) d = 1.0; }
  }
  return std::isnan(d) ? std::numeric_limits<double>::infinity() : d;
}

static std::string mst_query_name(const std::vector<std::string>& qnames, size_t q) {
  return qnames[q].empty() ? "query_" + std::to_string(q) : qnames[q];
}

bool write_mst_query_tsv(const std::string& path, const MstState& st, const std::vector<std::string>& qnames,
                         const std::vector<rtc_rep_hit>& hits, const std::vector<uint32_t>& per_query) {
  FILE* fp = fopen(path.c_str(), "w");
  if (!fp) { std::cerr << "ERROR: cannot open output file: " << path << std::endl; return false; }
  const std::vector<int> live = mst_live_index(st);
  const int wmode = mst_query_wmode(st);
  fprintf(fp, "#query\trank\trep_name\tdistance\tcluster_id\tcluster_size\n");
  size_t h = 0;
  for (size_t q = 0; q < qnames.size(); q++) {
    const std::string name = mst_query_name(qnames, q);
    if (per_query[q] == 0) fprintf(fp, "%s\t0\tno_match\t-1\t-1\t0\n", name.c_str());
    for (uint32_t r = 0; r < per_query[q]; r++, h++) {
      const rtc_rep_hit& x = hits[h];
      fprintf(fp, "%s\t%d\t%s\t%.6f\t%d\t%d\n", name.c_str(), (int)r + 1, st.rep_names[x.slot].c_str(),
              mst_query_distance(x.common, x.denom, wmode, st.kmer_size), live[x.slot], (int)st.clusters[x.slot].size());
    }
  }
  fclose(fp);
  return true;
}

bool write_mst_assign_tsv(const std::string& path, const MstState& st, const std::vector<std::string>& qnames,
                          const std::vector<rtc_rep_hit>& hits, const std::vector<uint32_t>& per_query, int* n_assigned) {
  FILE* fp = fopen(path.c_str(), "w");
  if (!fp) { std::cerr << "ERROR: cannot open output file: " << path << std::endl; return false; }
  const std::vector<int> live = mst_live_index(st);
  const int wmode = mst_query_wmode(st);
  fprintf(fp, "#query\tassigned_cluster\trep_name\tdistance\tcluster_size\tstatus\n");
  size_t h = 0;
  int assigned = 0;
  for (size_t q = 0; q < qnames.size(); q++) {
    const std::string name = mst_query_name(qnames, q);
    double d = 0.0;
    if (per_query[q]) d = mst_query_distance(hits[h].common, hits[h].denom, wmode, st.kmer_size);
    if (per_query[q] && d <= st.threshold) {  // MinHashMstAssign / KssdMstAssign: the top-1 hit within the state's threshold
      const uint32_t s = hits[h].slot;
      fprintf(fp, "%s\t%d\t%s\t%.6f\t%d\tassigned\n", name.c_str(), live[s], st.rep_names[s].c_str(), d, (int)st.clusters[s].size());
      assigned++;
    } else {
      fprintf(fp, "%s\t-1\tunassigned\t-1\t0\tnovel\n", name.c_str());
    }
    h += per_query[q];
  }
  fclose(fp);
  if (n_assigned) *n_assigned = assigned;
  return true;
}

void screen_report_text(const std::vector<std::string>& names, const std::vector<std::string>& rep_names, const std::vector<int>& cluster_id,
                        const std::vector<int>& cluster_size, const rtc_screen_hit* hits, size_t n_hits, const rtc_screen_sum* sums, int kmer_size,
                        double (*identity_fn)(uint32_t, uint32_t, int), std::string* tsv, std::string* summary) {
  char buf[256];
  if (tsv) *tsv = "#sample\trank\tcluster_id\trep_name\tcluster_size\tshared\trep_hashes\tcontainment\tidentity\tunique\tunique_share\n";
  if (summary) *summary = "#sample\thashes\tmatched\texplained\thits\tpicks\tunexplained_share\n";
  size_t h = 0;
  for (size_t q = 0; q < names.size(); q++) {
    const std::string name = mst_query_name(names, q);
    const rtc_screen_sum& s = sums[q];
    const size_t h0 = h;
    for (; h < n_hits && hits[h].query == q; h++) {
      if (!tsv) continue;
      const rtc_screen_hit& x = hits[h];
      *tsv += name + "\t" + (x.rank ? std::to_string(x.rank) : std::string("-")) + "\t" + std::to_string(cluster_id[x.slot]) + "\t" +
              rep_names[x.slot];
      snprintf(buf, sizeof buf, "\t%d\t%u\t%u\t%.6f\t%.6f\t%u\t%.6f\n", cluster_size[x.slot], x.common, x.size,
               x.size ? (double)x.common / (double)x.size : 0.0, identity_fn(x.common, x.size, kmer_size), x.unique,
               s.n_hashes ? (double)x.unique / (double)s.n_hashes : 0.0);
      *tsv += buf;
    }
    if (tsv && h == h0) *tsv += name + "\t0\t-1\tno_match\t0\t0\t0\t0.000000\t0.000000\t0\t0.000000\n";
    if (summary) {
      snprintf(buf, sizeof buf, "\t%u\t%u\t%u\t%u\t%u\t", s.n_hashes, s.n_matched, s.n_explained, s.n_hits, s.n_picks);
      *summary += name + buf;
      if (s.n_hashes) { snprintf(buf, sizeof buf, "%.6f\n", (double)(s.n_hashes - s.n_explained) / (double)s.n_hashes); *summary += buf; }
      else *summary += "-\n";
    }
  }
}

static bool write_mst_screen_file(const std::string& path, const MstState& st, const std::vector<std::string>& names,
                                  const std::vector<rtc_screen_hit>& hits, const std::vector<rtc_screen_sum>& sums,
                                  double (*identity_fn)(uint32_t, uint32_t, int), bool summary) {
  const std::vector<int> live = mst_live_index(st);
  std::vector<int> size(st.clusters.size());
  for (size_t r = 0; r < st.clusters.size(); r++) size[r] = (int)st.clusters[r].size();
  std::string text;
  screen_report_text(names, st.rep_names, live, size, hits.data(), hits.size(), sums.data(), st.kmer_size, identity_fn, summary ? nullptr : &text,
                     summary ? &text : nullptr);
  FILE* fp = fopen(path.c_str(), "w");
  if (!fp) { std::cerr << "ERROR: cannot open output file: " << path << std::endl; return false; }
  fwrite(text.data(), 1, text.size(), fp);
  fclose(fp);
  return true;
}
bool write_mst_screen_tsv(const std::string& path, const MstState& st, const std::vector<std::string>& names,
                          const std::vector<rtc_screen_hit>& hits, const std::vector<rtc_screen_sum>& sums,
                          double (*identity_fn)(uint32_t, uint32_t, int)) {
  return write_mst_screen_file(path, st, names, hits, sums, identity_fn, false);
}
bool write_mst_screen_summary_tsv(const std::string& path, const MstState& st, const std::vector<std::string>& names,
                                  const std::vector<rtc_screen_hit>& hits, const std::vector<rtc_screen_sum>& sums) {
  return write_mst_screen_file(path, st, names, hits, sums, nullptr, true);
}

void print_mst_state_clusters(const std::vector<std::vector<int>>& clusters, const std::vector<std::string>& member_names,
                              const std::vector<uint64_t>& member_lens, bool sketch_by_file, const std::string& output_file,
                              double threshold) {
  FILE* fp = fopen(output_file.c_str(), "w");
  if (!fp) { std::cerr << "ERROR: printMstStateClusterResult cannot open " << output_file << std::endl; return; }
  if (threshold >= 0.0) {
    fprintf(fp, "# Clustering threshold: %.6f\n", threshold);
    fprintf(fp, "# Total clusters: %zu\n", clusters.size());
    fprintf(fp, "#\n");
  }
  for (size_t c = 0; c < clusters.size(); c++) {
    fprintf(fp, "the cluster %zu is: \n", c);
    for (size_t j = 0; j < clusters[c].size(); j++) {
      const int id = clusters[c][j];
      const char* name = "N/A";
      uint64_t len = 0;
      if (id >= 0 && (size_t)id < member_names.size()) {
        name = member_names[id].c_str();
        len = (size_t)id < member_lens.size() ? member_lens[id] : 0;
      }
      if (sketch_by_file) fprintf(fp, "\t%5zu\t%6d\t%12lunt\t%20s\n", j, id, (unsigned long)len, name);
      else fprintf(fp, "\t%6zu\t%6d\t%12lunt\t%20s\n", j, id, (unsigned long)len, name);
    }
    fprintf(fp, "\n");
  }
  fclose(fp);
}

std::string current_date_time() {
  time_t now = time(0);
  struct tm tstruct = *localtime(&now);
  char buf[80];
  strftime(buf, sizeof(buf), "%Y_%m_%d_%H-%M-%S", &tstruct);
  return buf;
}

// ---- clust-dbscan --db: the model file ----
namespace {
const char DBSCAN_MODEL_MAGIC[9] = "RTCDBSM1";
struct ModelReader {
  const std::string& b;
  size_t at = 0;
  bool ok = true;
  template <typename T> T pod() {
    T v{};
    if (!ok || b.size() - at < sizeof(T)) { ok = false; return v; }
    memcpy(&v, b.data() + at, sizeof(T));
    at += sizeof(T);
    return v;
  }
  std::string str() {
    const uint32_t n = pod<uint32_t>();
    if (!ok || b.size() - at < n) { ok = false; return std::string(); }
    std::string s = b.substr(at, n);
    at += n;
    return s;
  }
  template <typename T> void vec(std::vector<T>& v, uint64_t n) {
    if (!ok || (b.size() - at) / sizeof(T) < n) { ok = false; return; }
    v.resize(n);
    if (n) memcpy(v.data(), b.data() + at, n * sizeof(T));
    at += n * sizeof(T);
  }
};
template <typename T> void model_put(std::string& o, const T& v) { o.append((const char*)&v, sizeof(T)); }
void model_put_str(std::string& o, const std::string& s) { model_put(o, (uint32_t)s.size()); o += s; }
// the genome records, the sketch lengths and the sketches of n genomes, shared by the model files
void model_put_genomes(std::string& o, const std::vector<GenomeInfo>& genomes, int width, const std::vector<std::vector<uint32_t>>& h32,
                       const std::vector<std::vector<uint64_t>>& h64) {
  const uint64_t n = genomes.size();
  for (uint64_t g = 0; g < n; g++) {
    const GenomeInfo& gi = genomes[g];
    model_put_str(o, gi.fileName); model_put_str(o, gi.seq0.name); model_put_str(o, gi.seq0.comment);
    model_put(o, (uint64_t)gi.seq0.length);
    model_put(o, gi.totalSeqLength);
  }
  for (uint64_t g = 0; g < n; g++) model_put(o, (uint32_t)(width == 8 ? h64[g].size() : h32[g].size()));
  for (uint64_t g = 0; g < n; g++) {
    if (width == 8) o.append((const char*)h64[g].data(), h64[g].size() * 8);
    else o.append((const char*)h32[g].data(), h32[g].size() * 4);
  }
}
void model_get_genomes(ModelReader& r, uint64_t n, int width, bool use64, std::vector<GenomeInfo>& genomes, std::vector<std::vector<uint32_t>>& h32,
                       std::vector<std::vector<uint64_t>>& h64) {
  for (uint64_t g = 0; r.ok && g < n; g++) {
    GenomeInfo gi;
    gi.id = (int)g;
    gi.fileName = r.str(); gi.seq0.name = r.str(); gi.seq0.comment = r.str();
    gi.seq0.length = (int)r.pod<uint64_t>();
    gi.totalSeqLength = r.pod<uint64_t>();
    gi.use64 = use64;
    genomes.push_back(gi);
  }
  std::vector<uint32_t> lens;
  r.vec(lens, n);
  if (width == 8) h64.resize(r.ok ? n : 0); else h32.resize(r.ok ? n : 0);
  for (uint64_t g = 0; r.ok && g < n; g++) {
    if (width == 8) r.vec(h64[g], lens[g]);
    else r.vec(h32[g], lens[g]);
  }
}
// the file through FILE.tmp and a rename
bool model_write(const std::string& path, const std::string& o) {
  const std::string tmp = path + ".tmp";
  {
    std::ofstream f(tmp, std::ios::binary | std::ios::trunc);
    if (!f) { std::cerr << "ERROR: --db " << path << ": cannot write " << tmp << std::endl; return false; }
    f.write(o.data(), (std::streamsize)o.size());
    f.close();
    if (!f) { std::cerr << "ERROR: --db " << path << ": writing " << tmp << " failed" << std::endl; remove(tmp.c_str()); return false; }
  }
  if (rename(tmp.c_str(), path.c_str()) != 0) { std::cerr << "ERROR: --db " << path << ": cannot rename " << tmp << std::endl; remove(tmp.c_str()); return false; }
  return true;
}
}  // namespace

bool save_dbscan_model(const std::string& path, const DbscanModel& m) {
  const uint64_t n = m.labels.size();
  std::string o(DBSCAN_MODEL_MAGIC, 8);
  const int32_t head[12] = {1, m.minhash ? 1 : 0, m.width, m.sketch_by_file ? 1 : 0, m.kmer_size, m.half_k, m.half_subk, m.drlevel,
                            m.sketch_size, m.min_pts, m.max_posting, m.n_clusters};
  o.append((const char*)head, sizeof head);
  model_put(o, m.min_len);
  model_put(o, n);
  model_put(o, m.eps);
  o.append((const char*)m.labels.data(), n * 4);
  o.append((const char*)m.core.data(), n);
  model_put_genomes(o, m.genomes, m.width, m.h32, m.h64);
  return model_write(path, o);
}

bool load_dbscan_model(const std::string& path, DbscanModel& m, std::string* why) {
  std::ifstream f(path, std::ios::binary);
  if (!f) { *why = "cannot open"; return false; }
  std::string blob((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  if (blob.size() < 8 || memcmp(blob.data(), DBSCAN_MODEL_MAGIC, 8) != 0) { *why = "is not a clust-dbscan model (bad magic)"; return false; }
  ModelReader r{blob};
  r.at = 8;
  int32_t head[12];
  for (int i = 0; i < 12; i++) head[i] = r.pod<int32_t>();
  if (!r.ok) { *why = "is truncated"; return false; }
  if (head[0] != 1) { *why = "has version " + std::to_string(head[0]) + ", this build reads version 1"; return false; }
  m = DbscanModel();
  m.minhash = head[1] == 1; m.width = head[2]; m.sketch_by_file = head[3] != 0; m.kmer_size = head[4]; m.half_k = head[5];
  m.half_subk = head[6]; m.drlevel = head[7]; m.sketch_size = head[8]; m.min_pts = head[9]; m.max_posting = head[10]; m.n_clusters = head[11];
  if ((head[1] != 0 && head[1] != 1) || (m.width != 4 && m.width != 8) || (m.minhash && m.width != 8)) {
    *why = "is not a clust-dbscan model (kind " + std::to_string(head[1]) + ", hash width " + std::to_string(m.width) + ")";
    return false;
  }
  m.min_len = r.pod<uint64_t>();
  const uint64_t n = r.pod<uint64_t>();
  m.eps = r.pod<double>();
  if (r.ok && n >= 0x7fffffffull) { *why = "is not a clust-dbscan model (" + std::to_string(n) + " genomes)"; return false; }
  r.vec(m.labels, n);
  r.vec(m.core, n);
  model_get_genomes(r, n, m.width, m.width == 8 && !m.minhash, m.genomes, m.h32, m.h64);
  if (!r.ok) { *why = "is truncated"; return false; }
  if (r.at != blob.size()) { *why = "has " + std::to_string(blob.size() - r.at) + " bytes after its end"; return false; }
  return true;
}

bool update_dbscan_model(DbscanModel& m, const std::vector<GenomeInfo>& add, const std::vector<std::vector<uint32_t>>* a32,
                         const std::vector<std::vector<uint64_t>>* a64, const std::vector<int32_t>& labels, const std::vector<uint8_t>& core,
                         int n_clusters) {
  const size_t n = m.labels.size() + add.size();
  if (labels.size() != n || core.size() != n) return false;
  if (m.width == 8 ? (!a64 || a64->size() != add.size()) : (!a32 || a32->size() != add.size())) return false;
  for (const GenomeInfo& g : add) {
    m.genomes.push_back(g);
    m.genomes.back().id = (int)m.genomes.size() - 1;
  }
  if (m.width == 8) m.h64.insert(m.h64.end(), a64->begin(), a64->end());
  else m.h32.insert(m.h32.end(), a32->begin(), a32->end());
  m.labels = labels;
  m.core = core;
  m.n_clusters = n_clusters;
  return true;
}

void print_dbscan_model_stats(const DbscanModel& m, std::ostream& os) {
  uint64_t noise = 0, core = 0;
  for (int32_t l : m.labels) noise += l < 0;
  for (uint8_t c : m.core) core += c != 0;
  os << "===== DBSCAN model =====" << std::endl
     << "  Kind:        " << (m.minhash ? "MinHash" : "KSSD") << std::endl
     << "  Hash width:  " << m.width << std::endl
     << "  Kmer size:   " << m.kmer_size << std::endl;
  if (m.minhash) os << "  Sketch size: " << m.sketch_size << std::endl;
  else os << "  Half k:      " << m.half_k << std::endl << "  Half subk:   " << m.half_subk << std::endl << "  Drlevel:     " << m.drlevel << std::endl;
  os << "  Min length:  " << m.min_len << std::endl
     << "  Eps:         " << m.eps << std::endl
     << "  MinPts:      " << m.min_pts << std::endl
     << "  Max posting: " << m.max_posting << std::endl
     << "  Genomes:     " << m.labels.size() << std::endl
     << "  Clusters:    " << m.n_clusters << std::endl
     << "  Noise:       " << noise << std::endl
     << "  Core points: " << core << std::endl
     << "========================" << std::endl;
}

uint32_t leiden_quantise_weight(double weight, const LeidenQuant& z) {
  const bool cpm = z.objective == 0;
  const double x = (cpm && z.scale) ? (weight - z.lo) / z.range : weight;
  long long q = llround(x * 1048576.0);
  if (!cpm && q < 1) q = 1;
  if (q < 1) return 0;
  return (uint32_t)std::min<long long>(q, 0xffffffffll);
}

bool leiden_quantiser(const double* weight, uint64_t m, int objective, LeidenQuant* z, double* w_min, double* w_max) {
  double lo = 1.0, hi = 0.0;
  for (uint64_t e = 0; e < m; e++) {
    if (weight[e] < lo) lo = weight[e];
    if (weight[e] > hi) hi = weight[e];
  }
  if (w_min) *w_min = lo;
  if (w_max) *w_max = hi;
  const bool cpm = objective == 0;
  const double range = hi - lo;
  const bool narrow = cpm && hi - lo < 0.5;
  z->objective = objective;
  z->scale = narrow && range > 1e-6;
  z->lo = lo;
  z->range = range;
  return narrow;
}

bool leiden_quantise(const uint32_t* u, const uint32_t* v, const double* weight, uint64_t m, int objective, std::vector<rtc_wedge>& out,
                     double* w_min, double* w_max) {
  out.clear();
  out.reserve(m);
  LeidenQuant z;
  const bool narrow = leiden_quantiser(weight, m, objective, &z, w_min, w_max);
  for (uint64_t e = 0; e < m; e++) {
    const uint32_t q = leiden_quantise_weight(weight[e], z);
    if (q < 1) continue;
    out.push_back(rtc_wedge{u[e], v[e], q});
  }
  return narrow;
}

bool leiden_model_sums(const rtc_wedge* records, uint64_t m, const int32_t* labels, uint32_t n, uint32_t n_clusters, LeidenModelSums& out) {
  out.k.assign(n, 0);
  out.tot.assign(n_clusters, 0);
  out.size.assign(n_clusters, 0);
  out.m2 = 0;
  for (uint64_t e = 0; e < m; e++) {
    if (records[e].u >= n || records[e].v >= n) return false;
    out.k[records[e].u] += records[e].q;  // u == v: both lines, 2q on the self entry
    out.k[records[e].v] += records[e].q;
  }
  for (uint32_t p = 0; p < n; p++) {
    if (labels[p] < 0 || (uint32_t)labels[p] >= n_clusters) return false;
    out.tot[labels[p]] += out.k[p];
    out.size[labels[p]]++;
    out.m2 += out.k[p];
  }
  return true;
}

void leiden_assign_weights(const rtc_qedge* edges, uint64_t m, const uint32_t* model_sizes, const uint32_t* query_sizes, int kmer_size,
                           double (*weight_fn)(uint32_t, uint32_t, uint32_t, int), const LeidenQuant& z, int threads, std::vector<rtc_wedge>& out) {
  std::vector<uint32_t> q(m);
  const uint64_t T = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(threads, 1), (m + 4095) / 4096));
  auto work = [&](uint64_t t) {
    for (uint64_t e = m * t / T; e < m * (t + 1) / T; e++)
      q[e] = leiden_quantise_weight(weight_fn(edges[e].common, query_sizes[edges[e].q], model_sizes[edges[e].p], kmer_size), z);
  };
  std::vector<std::thread> pool;
  for (uint64_t t = 1; t < T; t++) pool.emplace_back(work, t);
  work(0);
  for (std::thread& th : pool) th.join();
  out.clear();
  out.reserve(m);
  for (uint64_t e = 0; e < m; e++)
    if (q[e]) out.push_back(rtc_wedge{edges[e].q, edges[e].p, q[e]});
}

// ---- clust-leiden --db: the model file ----
namespace {
const char LEIDEN_MODEL_MAGIC[9] = "RTCLDNM1";
}

bool save_leiden_model(const std::string& path, const LeidenModel& m) {
  const uint64_t n = m.labels.size();
  std::string o(LEIDEN_MODEL_MAGIC, 8);
  const int32_t head[12] = {1, m.algorithm, m.objective, m.width, m.sketch_by_file ? 1 : 0, m.kmer_size, m.half_k, m.half_subk, m.drlevel, m.knn,
                            m.n_clusters, m.scale ? 1 : 0};
  o.append((const char*)head, sizeof head);
  model_put(o, m.min_len);
  model_put(o, n);
  model_put(o, m.threshold);
  model_put(o, m.resolution);
  model_put(o, m.lo);
  model_put(o, m.range);
  model_put(o, m.m2);
  o.append((const char*)m.labels.data(), n * 4);
  o.append((const char*)m.tot.data(), m.tot.size() * 8);
  model_put_genomes(o, m.genomes, m.width, m.h32, m.h64);
  return model_write(path, o);
}

bool load_leiden_model(const std::string& path, LeidenModel& m, std::string* why) {
  std::ifstream f(path, std::ios::binary);
  if (!f) { *why = "cannot open"; return false; }
  std::string blob((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  if (blob.size() < 8 || memcmp(blob.data(), LEIDEN_MODEL_MAGIC, 8) != 0) { *why = "is not a clust-leiden model (bad magic)"; return false; }
  ModelReader r{blob};
  r.at = 8;
  int32_t head[12];
  for (int i = 0; i < 12; i++) head[i] = r.pod<int32_t>();
  if (!r.ok) { *why = "is truncated"; return false; }
  if (head[0] != 1) { *why = "has version " + std::to_string(head[0]) + ", this build reads version 1"; return false; }
  m = LeidenModel();
  m.algorithm = head[1]; m.objective = head[2]; m.width = head[3]; m.sketch_by_file = head[4] != 0; m.kmer_size = head[5]; m.half_k = head[6];
  m.half_subk = head[7]; m.drlevel = head[8]; m.knn = head[9]; m.n_clusters = head[10]; m.scale = head[11] != 0;
  if ((m.algorithm != 0 && m.algorithm != 1) || (m.objective != 0 && m.objective != 1) || (m.width != 4 && m.width != 8) || m.knn < 0 ||
      m.n_clusters < 0) {
    *why = "is not a clust-leiden model (algorithm " + std::to_string(m.algorithm) + ", objective " + std::to_string(m.objective) + ", hash width " +
           std::to_string(m.width) + ")";
    return false;
  }
  m.min_len = r.pod<uint64_t>();
  const uint64_t n = r.pod<uint64_t>();
  m.threshold = r.pod<double>();
  m.resolution = r.pod<double>();
  m.lo = r.pod<double>();
  m.range = r.pod<double>();
  m.m2 = r.pod<uint64_t>();
  if (r.ok && (n >= 0x7fffffffull || (uint64_t)m.n_clusters > n)) {
    *why = "is not a clust-leiden model (" + std::to_string(n) + " genomes, " + std::to_string(m.n_clusters) + " clusters)";
    return false;
  }
  r.vec(m.labels, n);
  r.vec(m.tot, (uint64_t)m.n_clusters);
  model_get_genomes(r, n, m.width, m.width == 8, m.genomes, m.h32, m.h64);
  if (!r.ok) { *why = "is truncated"; return false; }
  if (r.at != blob.size()) { *why = "has " + std::to_string(blob.size() - r.at) + " bytes after its end"; return false; }
  for (int32_t l : m.labels)
    if (l < 0 || l >= m.n_clusters) { *why = "is not a clust-leiden model (label " + std::to_string(l) + ")"; return false; }
  return true;
}

void print_leiden_model_stats(const LeidenModel& m, std::ostream& os) {
  std::vector<uint64_t> size((size_t)m.n_clusters, 0);
  for (int32_t l : m.labels) size[l]++;
  uint64_t largest = 0, single = 0;
  for (uint64_t s : size) { largest = std::max(largest, s); single += s == 1; }
  os << "===== Leiden model =====" << std::endl
     << "  Algorithm:   " << (m.algorithm == 1 ? "Leiden" : "Louvain") << std::endl
     << "  Objective:   " << (m.objective == 0 ? "cpm" : "modularity") << std::endl
     << "  Hash width:  " << m.width << std::endl
     << "  Kmer size:   " << m.kmer_size << std::endl
     << "  Half k:      " << m.half_k << std::endl << "  Half subk:   " << m.half_subk << std::endl << "  Drlevel:     " << m.drlevel << std::endl
     << "  Min length:  " << m.min_len << std::endl
     << "  Threshold:   " << m.threshold << std::endl
     << "  Resolution:  " << m.resolution << std::endl
     << "  Knn:         " << m.knn << std::endl;
  if (m.objective == 0) {
    os << "  Weights:     ";
    if (m.scale) os << "scaled from [" << m.lo << ", " << m.lo + m.range << "]" << std::endl;
    else os << "as they are" << std::endl;
  } else {
    os << "  Total weight: " << m.m2 << std::endl;
  }
  os << "  Genomes:     " << m.labels.size() << std::endl
     << "  Clusters:    " << m.n_clusters << std::endl
     << "  Largest:     " << largest << std::endl
     << "  Singletons:  " << single << std::endl
     << "========================" << std::endl;
}

}  // namespace rtc
