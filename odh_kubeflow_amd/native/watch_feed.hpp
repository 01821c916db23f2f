// Byte-level framing of a watch response body: HTTP/1.1 body bytes in, JSON lines out.
//
// Python-free (objcore.cpp's WatchStore decodes the lines; tests/native/watch_feed_check.cpp
// drives the framer alone).  A body is chunked (chunk extensions, the terminal chunk and its
// trailer included), of a known Content-Length, or delimited by the end of the connection.
// Bytes arrive cut anywhere: the framer keeps what is incomplete between calls, so feeding a
// body whole, byte by byte or split at any offsets gives the same lines.  Blank (keep-alive)
// lines are dropped.  A complete line that lies inside one call's bytes is handed over in
// place, without a copy.
#pragma once

#include <cstddef>
#include <cstring>
#include <stdexcept>
#include <string>

namespace watchfeed {

struct FrameError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

constexpr long long kChunked = -2;   // Transfer-Encoding: chunked
constexpr long long kUntilEof = -3;  // delimited by the server closing the connection
// a chunk-size line (size and extensions) longer than this is not one
constexpr size_t kMaxSizeLine = 4096;
// 15 hex digits: the largest chunk size taken (fits a signed 64-bit count with room to spare)
constexpr int kMaxSizeDigits = 15;

inline bool is_blank(const char* s, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    const char c = s[i];
    if (c != ' ' && c != '\t' && c != '\r' && c != '\n' && c != '\v' && c != '\f') return false;
  }
  return true;
}

class Framer {
 public:
  // want: kChunked, kUntilEof, or the Content-Length
  void begin(long long want) {
    if (want < kUntilEof) throw FrameError("bad body length");
    want_ = want;
    state_ = want == kChunked ? kSize : want == 0 ? kDone : kBody;
    left_ = want > 0 ? want : 0;
    head_.clear();
    line_.clear();
  }

  bool done() const { return state_ == kDone; }
  // the bytes of the last, incomplete line
  const std::string& partial() const { return line_; }

  // Consume ``n`` bytes; on_line(const char*, size_t) -> bool is called with every complete,
  // non-blank line (its newline removed) and returns false to stop: the rest of the body is
  // then dropped and the framer is done.  Bytes after the end of the body are ignored.
  template <class F>
  void feed(const char* p, size_t n, F&& on_line) {
    const char* end = p + n;
    while (p < end && state_ != kDone) {
      switch (state_) {
        case kSize:
        case kTrailer: {
          const char* nl = static_cast<const char*>(std::memchr(p, '\n', static_cast<size_t>(end - p)));
          const size_t take = static_cast<size_t>((nl ? nl : end) - p);
          if (head_.size() + take > kMaxSizeLine) throw FrameError("chunk header line too long");
          head_.append(p, take);
          p += take;
          if (!nl) break;
          ++p;
          if (head_.empty() || head_.back() != '\r') throw FrameError("chunk header line without CRLF");
          head_.pop_back();
          if (state_ == kTrailer) {
            if (head_.empty()) state_ = kDone;  // the empty line that ends the trailer
          } else {
            left_ = parse_size(head_);
            state_ = left_ == 0 ? kTrailer : kData;
          }
          head_.clear();
          break;
        }
        case kData:
        case kBody: {
          size_t span = static_cast<size_t>(end - p);
          if (state_ == kData || want_ >= 0) {
            if (static_cast<unsigned long long>(left_) < span) span = static_cast<size_t>(left_);
            left_ -= static_cast<long long>(span);
          }
          const bool more = lines(p, span, on_line);
          p += span;
          if (!more) {
            state_ = kDone;
          } else if (state_ == kData) {
            if (left_ == 0) state_ = kDataCr;
          } else if (want_ >= 0 && left_ == 0) {
            state_ = kDone;
          }
          break;
        }
        case kDataCr:
          if (*p != '\r') throw FrameError("no CRLF after the chunk data");
          ++p;
          state_ = kDataLf;
          break;
        case kDataLf:
          if (*p != '\n') throw FrameError("no CRLF after the chunk data");
          ++p;
          state_ = kSize;
          break;
        case kDone:
          break;
      }
    }
  }

 private:
  enum State { kSize, kData, kDataCr, kDataLf, kTrailer, kBody, kDone };

  static long long parse_size(const std::string& s) {
    size_t i = 0, n = s.size();
    const size_t semi = s.find(';');
    if (semi != std::string::npos) n = semi;  // chunk extensions
    while (i < n && (s[i] == ' ' || s[i] == '\t')) ++i;
    while (n > i && (s[n - 1] == ' ' || s[n - 1] == '\t')) --n;
    if (i == n) throw FrameError("empty chunk size");
    if (n - i > static_cast<size_t>(kMaxSizeDigits)) throw FrameError("chunk size too large");
    long long v = 0;
    for (; i < n; ++i) {
      const char c = s[i];
      int d;
      if (c >= '0' && c <= '9') d = c - '0';
      else if (c >= 'a' && c <= 'f') d = c - 'a' + 10;
      else if (c >= 'A' && c <= 'F') d = c - 'A' + 10;
      else throw FrameError("bad chunk size");
      v = v * 16 + d;
    }
    return v;
  }

  // split body bytes into lines; false once on_line asked to stop
  template <class F>
  bool lines(const char* p, size_t n, F&& on_line) {
    const char* end = p + n;
    while (p < end) {
      const char* nl = static_cast<const char*>(std::memchr(p, '\n', static_cast<size_t>(end - p)));
      if (!nl) {
        line_.append(p, static_cast<size_t>(end - p));
        return true;
      }
      bool more = true;
      if (line_.empty()) {
        const size_t len = static_cast<size_t>(nl - p);
        if (!is_blank(p, len)) more = on_line(p, len);
      } else {
        line_.append(p, static_cast<size_t>(nl - p));
        // moved out first: on_line may throw, and the line must not be seen twice
        std::string whole;
        whole.swap(line_);
        if (!is_blank(whole.data(), whole.size())) more = on_line(whole.data(), whole.size());
      }
      p = nl + 1;
      if (!more) return false;
    }
    return true;
  }

  long long want_ = kUntilEof;
  State state_ = kBody;
  long long left_ = 0;
  std::string head_;  // a chunk-size or trailer line in progress
  std::string line_;  // a body line in progress
};

}  // namespace watchfeed
