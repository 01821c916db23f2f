// Stand-alone check of the watch-body framer (odh_kubeflow_amd/native/watch_feed.hpp).
//
// A chunked body of 40 lines (a chunk extension, two lines in one chunk, one line over three
// chunks, blank keep-alive lines, a line of one byte and one of 1500, the terminal chunk with a
// trailer) is framed whole, byte by byte, cut in two at every offset and cut in five at 500
// seeded random places: the lines must be the ones the body was made of, every time.  Then
// bodies cut short, chunk sizes that are truncated, oversized or no numbers, a missing CRLF after
// the chunk data, Content-Length and EOF-delimited bodies, and a consumer that stops.
// Built plain and with -fsanitize=address,undefined by tests/test_watch_feed_native.py.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "watch_feed.hpp"

namespace {

long checks = 0;

#define CHECK(cond)                                                      \
  do {                                                                   \
    ++checks;                                                            \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                      \
    }                                                                    \
  } while (0)

using Lines = std::vector<std::string>;

std::string hex(size_t n) {
  char b[32];
  std::snprintf(b, sizeof b, "%zx", n);
  return b;
}

std::string chunk(const std::string& data, const std::string& ext = "") {
  return hex(data.size()) + ext + "\r\n" + data + "\r\n";
}

struct Result {
  Lines lines;
  bool done = false;
  bool failed = false;
  std::string partial;
};

// frame ``body`` cut at ``cuts`` (ascending offsets); every piece is copied to a buffer of its
// exact size, so that a read past a piece's end is one past an allocation
Result run(const std::string& body, const std::vector<size_t>& cuts, long long want = watchfeed::kChunked,
           size_t stop_after = 0) {
  Result r;
  watchfeed::Framer f;
  f.begin(want);
  size_t a = 0;
  try {
    for (size_t i = 0; i <= cuts.size(); ++i) {
      const size_t b = i < cuts.size() ? cuts[i] : body.size();
      std::vector<char> piece(body.begin() + static_cast<long>(a), body.begin() + static_cast<long>(b));
      f.feed(piece.data(), piece.size(), [&](const char* s, size_t n) {
        r.lines.emplace_back(s, n);
        return stop_after == 0 || r.lines.size() < stop_after;
      });
      a = b;
    }
  } catch (const watchfeed::FrameError&) {
    r.failed = true;
  }
  r.done = f.done();
  r.partial = f.partial();
  return r;
}

bool fails(const std::string& body) {
  // whole, and byte by byte: a fault is one wherever the bytes are cut
  std::vector<size_t> every;
  for (size_t i = 1; i < body.size(); ++i) every.push_back(i);
  const Result whole = run(body, {}), bytes = run(body, every);
  CHECK(whole.failed == bytes.failed);
  CHECK(whole.lines == bytes.lines);
  return whole.failed;
}

}  // namespace

int main() {
  std::mt19937 rnd(20240);
  Lines want;
  for (int i = 0; i < 40; ++i) {
    const size_t n = i == 7 ? 1 : i == 11 ? 1500 : 20 + rnd() % 120;
    std::string s = "{\"n\":" + std::to_string(i) + ",\"pad\":\"";
    while (s.size() < n) s.push_back(static_cast<char>('a' + rnd() % 26));
    if (i == 7) s = "7";
    else s += "\"}";
    if (i % 9 == 0) s += "\r";  // a line may end in CRLF: the CR stays with the line
    want.push_back(s);
  }
  std::string body = chunk(want[0] + "\n", ";ext=1;q=\"x y\"");
  body += chunk(want[1] + "\n" + want[2] + "\n");
  body += chunk("\n") + chunk(" \t\r\n");  // keep-alives
  const std::string l3 = want[3] + "\n";
  body += chunk(l3.substr(0, 5)) + chunk(l3.substr(5, 9)) + chunk(l3.substr(14));
  for (size_t i = 4; i < want.size(); ++i) body += chunk(want[i] + "\n", i % 5 == 0 ? " ; a=b" : "");
  const size_t before_end = body.size();
  body += "0\r\nX-Trailer: done\r\nOther: 1\r\n\r\n";

  // whole, byte by byte, every 2-split, 500 random 5-splits
  {
    const Result r = run(body, {});
    CHECK(r.lines == want && r.done && !r.failed && r.partial.empty());
    std::vector<size_t> every;
    for (size_t i = 1; i < body.size(); ++i) every.push_back(i);
    const Result b = run(body, every);
    CHECK(b.lines == want && b.done && !b.failed);
    for (size_t i = 0; i <= body.size(); ++i) {
      const Result s = run(body, {i});
      CHECK(s.lines == want && s.done && !s.failed);
    }
    for (int k = 0; k < 500; ++k) {
      std::vector<size_t> cuts;
      for (int j = 0; j < 4; ++j) cuts.push_back(rnd() % (body.size() + 1));
      std::sort(cuts.begin(), cuts.end());
      const Result s = run(body, cuts);
      CHECK(s.lines == want && s.done && !s.failed);
    }
  }
  // a body cut short anywhere: a prefix of the lines, not done, no fault; bytes after the end: ignored
  for (size_t n = 0; n < body.size(); n += 7) {
    const Result r = run(body.substr(0, n), {n / 2});
    CHECK(!r.failed && r.done == false && r.lines.size() <= want.size());
    CHECK(Lines(want.begin(), want.begin() + static_cast<long>(r.lines.size())) == r.lines);
  }
  {
    const Result r = run(body + "HTTP/1.1 200 OK\r\n\r\nzz\r\n", {before_end});
    CHECK(r.lines == want && r.done && !r.failed);
  }
  // the terminal chunk without a trailer; the trailer cut short
  CHECK(run(chunk("a\n") + "0\r\n\r\n", {}).done);
  CHECK(!run(chunk("a\n") + "0\r\n", {}).done);
  CHECK(!run(chunk("a\n") + "0\r\nX: y\r\n", {}).done);
  // chunk sizes
  CHECK(!fails("A\r\n123456789\n\r\n0\r\n\r\n"));
  CHECK(!fails("  00a \r\n123456789\n\r\n0\r\n\r\n"));
  CHECK(fails("\r\nabc\r\n"));                      // truncated to nothing
  CHECK(fails(";ext\r\nabc\r\n"));
  CHECK(fails("zz\r\nabc\r\n"));
  CHECK(fails("-5\r\nabcde\r\n"));
  CHECK(fails("0x5\r\nabcde\r\n"));
  CHECK(fails("5 5\r\nabcde\r\n"));
  CHECK(fails("5\nabcde\r\n"));                     // LF alone after the size
  CHECK(fails("1234567890abcdef\r\nabc"));          // 16 digits: oversized
  CHECK(!fails("123456789abcdef\r\nabc"));          // 15: taken (and waits for the data)
  CHECK(fails("ffffffffffffffffffffffffffffffff\r\nabc"));
  CHECK(fails(std::string(5000, '1') + "\r\n"));    // a size line with no end in sight
  CHECK(fails("5;" + std::string(5000, 'x')));
  CHECK(fails("0\r\n" + std::string(5000, 'x')));   // nor a trailer line
  // the CRLF after the chunk data
  CHECK(fails("5\r\nabcd\nXY\r\n"));
  CHECK(fails("5\r\nabcd\n\rY\r\n"));
  CHECK(fails("5\r\nabcd\n\n"));
  {
    const Result r = run("5\r\nabcd\nXY", {});
    CHECK(r.failed && r.lines == Lines{"abcd"});  // the line before the fault was complete
  }
  // Content-Length and EOF-delimited bodies
  {
    const std::string plain = want[0] + "\n\n" + want[1] + "\n" + want[2];
    for (size_t i = 0; i <= plain.size(); ++i) {
      Result r = run(plain + "next", {i}, static_cast<long long>(plain.size()));
      CHECK((r.lines == Lines{want[0], want[1]}) && r.done && r.partial == want[2]);
      r = run(plain, {i}, watchfeed::kUntilEof);
      CHECK((r.lines == Lines{want[0], want[1]}) && !r.done && r.partial == want[2]);
    }
    CHECK(run("", {}, 0).done);
    watchfeed::Framer f;
    bool threw = false;
    try {
      f.begin(-7);
    } catch (const watchfeed::FrameError&) {
      threw = true;
    }
    CHECK(threw);
  }
  // a consumer that stops (an ERROR event): nothing after it, and the framer is done
  for (size_t i = 0; i <= body.size(); i += 3) {
    const Result r = run(body, {i}, watchfeed::kChunked, 5);
    CHECK(r.lines == Lines(want.begin(), want.begin() + 5) && r.done && !r.failed);
  }
  std::printf("OK %ld checks\n", checks);
  return 0;
}
