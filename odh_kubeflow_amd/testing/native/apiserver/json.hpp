// Minimal JSON DOM for the native apiserver: a compact copy-on-write tree, strict parser,
// compact serializer (shortest round-trip doubles), deep equality that ignores object key
// order.  Kubernetes objects are small (KiB), so objects are vectors of members with linear
// lookup — faster than hashing at these sizes and order-preserving.
//
// A Value is 16 bytes: a tag and either a scalar, a string of up to 14 bytes, or a pointer to an
// atomically reference-counted payload (longer string, array, object).  A payload is never changed while it is
// shared: copying a Value bumps the count, and the mutators (operator[], erase, get_mut,
// arr_mut, obj_mut) first detach the ONE level they change — a private copy of that level's
// vector whose elements still share their own payloads.  So a stored object can be "copied"
// and patched for the price of the path from the root to the change, and two Values on the
// same payload compare equal without a walk (same()).  Reading (get, arr, obj, s, dump, ==)
// never detaches and is safe from any number of threads on a shared tree; a Value that is
// being mutated belongs to one thread, as with any container.
//
// Object keys of up to 15 bytes live inside the member.  Longer keys are interned in a table
// that counts references per key and drops a key with its last member, so client-chosen keys
// (labels, annotations) cannot make it grow: it holds exactly the long keys of the live trees.
#pragma once

#include <atomic>
#include <charconv>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <iterator>
#include <new>
#include <mutex>
#include <stdexcept>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

namespace kj {

enum class T : uint8_t { Null, Bool, Int, Double, String, Array, Object };

namespace detail {

// one interned long key: `s` never changes, `rc` counts the Keys that point here
struct KeyEnt {
  std::atomic<uint32_t> rc{1};
  std::string s;
};

struct KeyShard {
  std::mutex mu;
  std::unordered_map<std::string_view, KeyEnt*> map;  // the view is into the entry's own string
};
constexpr size_t kKeyShards = 32;

// never destroyed: Values in objects of static storage duration release keys at exit
inline KeyShard* key_shards() {
  static KeyShard* t = new KeyShard[kKeyShards];
  return t;
}
inline KeyShard& key_shard(std::string_view s) { return key_shards()[std::hash<std::string_view>{}(s) % kKeyShards]; }

inline KeyEnt* key_intern(std::string_view s) {
  KeyShard& sh = key_shard(s);
  std::lock_guard<std::mutex> g(sh.mu);
  auto it = sh.map.find(s);
  if (it != sh.map.end()) {
    // an entry in the map has rc >= 1: the drop to zero happens under this lock, with the erase
    it->second->rc.fetch_add(1, std::memory_order_relaxed);
    return it->second;
  }
  KeyEnt* e = new KeyEnt;
  e->s.assign(s.data(), s.size());
  sh.map.emplace(std::string_view(e->s), e);
  return e;
}

inline void key_release(KeyEnt* e) {
  uint32_t n = e->rc.load(std::memory_order_relaxed);
  while (n > 1)
    if (e->rc.compare_exchange_weak(n, n - 1, std::memory_order_acq_rel, std::memory_order_relaxed)) return;
  // possibly the last reference: decided under the shard's lock, so that key_intern never
  // finds an entry on its way out
  KeyShard& sh = key_shard(e->s);
  std::unique_lock<std::mutex> g(sh.mu);
  if (e->rc.fetch_sub(1, std::memory_order_acq_rel) != 1) return;
  sh.map.erase(std::string_view(e->s));
  g.unlock();
  delete e;
}

// long keys interned right now (the tests: nothing is held once every tree is gone)
inline size_t keys_interned() {
  size_t n = 0;
  for (size_t k = 0; k < kKeyShards; ++k) {
    std::lock_guard<std::mutex> g(key_shards()[k].mu);
    n += key_shards()[k].map.size();
  }
  return n;
}

}  // namespace detail

// An object member's name: up to 15 bytes inline (zero padded, length in the last byte), longer
// ones a counted reference to the interned string.  Either way two equal keys hold equal bits.
class Key {
 public:
  static constexpr size_t kInline = 15;
  Key() { w_[0] = w_[1] = 0; }
  explicit Key(std::string_view s) {
    w_[0] = w_[1] = 0;
    if (s.size() <= kInline) {
      std::memcpy(bytes(), s.data(), s.size());
      bytes()[15] = (char)s.size();
    } else {
      detail::KeyEnt* e = detail::key_intern(s);
      std::memcpy(bytes(), &e, sizeof(e));
      bytes()[15] = (char)kLong;
    }
  }
  Key(const Key& o) {
    w_[0] = o.w_[0];
    w_[1] = o.w_[1];
    if (is_long()) ent()->rc.fetch_add(1, std::memory_order_relaxed);
  }
  Key(Key&& o) noexcept {
    w_[0] = o.w_[0];
    w_[1] = o.w_[1];
    o.w_[0] = o.w_[1] = 0;
  }
  Key& operator=(Key o) noexcept {
    std::swap(w_[0], o.w_[0]);
    std::swap(w_[1], o.w_[1]);
    return *this;
  }
  ~Key() {
    if (is_long()) detail::key_release(ent());
  }

  std::string_view sv() const {
    if (is_long()) return ent()->s;
    return std::string_view(bytes(), (size_t)(unsigned char)bytes()[15]);
  }
  operator std::string_view() const { return sv(); }
  std::string str() const { return std::string(sv()); }
  bool empty() const { return sv().empty(); }
  size_t size() const { return sv().size(); }
  char operator[](size_t n) const { return sv()[n]; }

  friend bool operator==(const Key& a, const Key& b) { return a.w_[0] == b.w_[0] && a.w_[1] == b.w_[1]; }
  friend bool operator!=(const Key& a, const Key& b) { return !(a == b); }
  friend bool operator==(const Key& a, std::string_view b) { return a.sv() == b; }
  friend bool operator!=(const Key& a, std::string_view b) { return a.sv() != b; }

 private:
  static constexpr unsigned char kLong = 0xFF;
  uint64_t w_[2];
  char* bytes() { return reinterpret_cast<char*>(w_); }
  const char* bytes() const { return reinterpret_cast<const char*>(w_); }
  bool is_long() const { return (unsigned char)bytes()[15] == kLong; }
  detail::KeyEnt* ent() const {
    detail::KeyEnt* e;
    std::memcpy(&e, bytes(), sizeof(e));
    return e;
  }
};

struct Member;
struct StrP;
struct ArrP;
struct ObjP;

struct Value {
  // Read t / b / i / d freely (b / i / d after checking `t`: they mean something for Bool / Int /
  // Double only); write a Value only through the factories and the mutators below.  Two views
  // of the same 16 bytes: the tag, then either a short string's length and bytes, or — in the
  // second word — the scalar or the payload pointer.  Bytes that a value does not use are zero.
  static constexpr size_t kInlineStr = 14;
  static constexpr uint8_t kHeapStr = 0xFF;
  union {
    struct {
      T t;
      uint8_t sn_;          // String: its length when the bytes are in sc_, kHeapStr when in *sp_
      char sc_[kInlineStr];
    };
    struct {
      uint64_t w0_;
      union {
        bool b;
        int64_t i;
        double d;
        StrP* sp_;
        ArrP* ap_;  // nullptr: the empty array
        ObjP* op_;  // nullptr: the empty object
        uint64_t w1_;
      };
    };
  };

  Value() : w0_(0), w1_(0) {}
  Value(const Value& o);
  Value(Value&& o) noexcept : w0_(o.w0_), w1_(o.w1_) { o.w0_ = o.w1_ = 0; }
  Value& operator=(Value o) noexcept {
    std::swap(w0_, o.w0_);
    std::swap(w1_, o.w1_);
    return *this;
  }
  ~Value() {
    if (t >= T::String) drop();
  }

  static Value null() { return Value(); }
  static Value boolean(bool v) { Value x; x.t = T::Bool; x.b = v; return x; }
  static Value integer(int64_t v) { Value x; x.t = T::Int; x.i = v; return x; }
  static Value number(double v) { Value x; x.t = T::Double; x.d = v; return x; }
  static Value str(std::string_view v);
  static Value array() { Value x; x.t = T::Array; return x; }
  static Value object() { Value x; x.t = T::Object; return x; }
  // built in one allocation each from finished elements (the parser)
  static Value array_of(std::vector<Value>&& v);
  static Value object_of(std::vector<Member>&& v);

  bool is_null() const { return t == T::Null; }
  bool is_obj() const { return t == T::Object; }
  bool is_arr() const { return t == T::Array; }
  bool is_str() const { return t == T::String; }
  int64_t int_or(int64_t dflt) const { return t == T::Int ? i : dflt; }

  // const views: never detach; the empty string / vector for a value of another type.  s() is
  // a view into the value itself (a short string) or its payload: valid while the value is
  // neither changed nor moved
  std::string_view s() const;
  const std::vector<Value>& arr() const;
  const std::vector<Member>& obj() const;
  // explicit mutable access: this level becomes private to this Value first (and the value an
  // array / object if it was of another type)
  std::vector<Value>& arr_mut();
  std::vector<Member>& obj_mut();

  // both on the same payload (or equal scalars of the same type): equal without a walk.  False
  // says nothing.
  bool same(const Value& o) const {
    if (t != o.t) return false;
    switch (t) {
      case T::Null: return true;
      case T::Bool: return b == o.b;
      case T::Double: return d == o.d;
      case T::String: return w0_ == o.w0_ && w1_ == o.w1_;  // the same bytes, or the same payload
      default: return i == o.i;  // Int, or the payload pointer
    }
  }

  // object access
  const Value* get(std::string_view k) const;
  const Value* get(const Key& k) const;
  Value* get_mut(std::string_view k);      // detaches this level
  Value& operator[](std::string_view k);   // insert null if absent (turns a non-object into an object)
  bool erase(std::string_view k);          // detaches only when the member is there
  std::string str_or(std::string_view k, const std::string& dflt = "") const {
    const Value* v = get(k);
    return v && v->t == T::String ? std::string(v->s()) : dflt;
  }
  // the string member `k`, or "" — a view into the tree, valid while the tree is
  std::string_view sv(std::string_view k) const {
    const Value* v = get(k);
    return v && v->t == T::String ? v->s() : std::string_view();
  }
  const Value* path(std::initializer_list<std::string_view> ks) const {
    const Value* cur = this;
    for (auto k : ks) {
      if (!cur || cur->t != T::Object) return nullptr;
      cur = cur->get(k);
    }
    return cur;
  }

 private:
  void drop();
};

struct Member {
  Key k;
  Value v;
};

// a string of more than 14 bytes: the count, the length and, right behind them, the bytes
struct StrP {
  std::atomic<uint32_t> rc{1};
  uint32_t len = 0;
  char* data() { return reinterpret_cast<char*>(this + 1); }
  const char* data() const { return reinterpret_cast<const char*>(this + 1); }
  static StrP* make(std::string_view v) {
    StrP* p = new (::operator new(sizeof(StrP) + v.size())) StrP;
    p->len = (uint32_t)v.size();
    std::memcpy(p->data(), v.data(), v.size());
    return p;
  }
  static void free(StrP* p) {
    p->~StrP();
    ::operator delete(p);
  }
};
struct ArrP {
  std::atomic<uint32_t> rc{1};
  std::vector<Value> v;
};
struct ObjP {
  std::atomic<uint32_t> rc{1};
  std::vector<Member> v;
};

static_assert(sizeof(Value) == 16, "a Value is a tag and one word");
static_assert(sizeof(Member) == 32, "a member is its key and its value");

inline Value::Value(const Value& o) : w0_(o.w0_), w1_(o.w1_) {
  switch (t) {
    case T::String: if (sn_ == kHeapStr) sp_->rc.fetch_add(1, std::memory_order_relaxed); break;
    case T::Array: if (ap_) ap_->rc.fetch_add(1, std::memory_order_relaxed); break;
    case T::Object: if (op_) op_->rc.fetch_add(1, std::memory_order_relaxed); break;
    default: break;
  }
}

inline void Value::drop() {
  switch (t) {
    case T::String:
      if (sn_ == kHeapStr && sp_->rc.fetch_sub(1, std::memory_order_acq_rel) == 1) StrP::free(sp_);
      break;
    case T::Array:
      if (ap_ && ap_->rc.fetch_sub(1, std::memory_order_acq_rel) == 1) delete ap_;
      break;
    case T::Object:
      if (op_ && op_->rc.fetch_sub(1, std::memory_order_acq_rel) == 1) delete op_;
      break;
    default: break;
  }
}

inline Value Value::str(std::string_view v) {
  Value x;
  if (v.size() <= kInlineStr) {
    x.sn_ = (uint8_t)v.size();
    std::memcpy(x.sc_, v.data(), v.size());
  } else {
    x.sp_ = StrP::make(v);
    x.sn_ = kHeapStr;
  }
  x.t = T::String;
  return x;
}
inline Value Value::array_of(std::vector<Value>&& v) {
  Value x;
  x.t = T::Array;
  x.ap_ = nullptr;
  if (!v.empty()) {
    x.ap_ = new ArrP;
    x.ap_->v = std::move(v);
  }
  return x;
}
inline Value Value::object_of(std::vector<Member>&& v) {
  Value x;
  x.t = T::Object;
  x.op_ = nullptr;
  if (!v.empty()) {
    x.op_ = new ObjP;
    x.op_->v = std::move(v);
  }
  return x;
}

inline std::string_view Value::s() const {
  if (t != T::String) return std::string_view();
  return sn_ == kHeapStr ? std::string_view(sp_->data(), sp_->len) : std::string_view(sc_, sn_);
}
inline const std::vector<Value>& Value::arr() const {
  static const std::vector<Value> empty;
  return t == T::Array && ap_ ? ap_->v : empty;
}
inline const std::vector<Member>& Value::obj() const {
  static const std::vector<Member> empty;
  return t == T::Object && op_ ? op_->v : empty;
}

inline std::vector<Value>& Value::arr_mut() {
  if (t != T::Array) *this = Value::array();
  if (!ap_) {
    ap_ = new ArrP;
  } else if (ap_->rc.load(std::memory_order_acquire) != 1) {
    ArrP* n = new ArrP;
    n->v = ap_->v;  // the elements still share their payloads
    if (ap_->rc.fetch_sub(1, std::memory_order_acq_rel) == 1) delete ap_;
    ap_ = n;
  }
  return ap_->v;
}
inline std::vector<Member>& Value::obj_mut() {
  if (t != T::Object) *this = Value::object();
  if (!op_) {
    op_ = new ObjP;
  } else if (op_->rc.load(std::memory_order_acquire) != 1) {
    ObjP* n = new ObjP;
    n->v = op_->v;
    if (op_->rc.fetch_sub(1, std::memory_order_acq_rel) == 1) delete op_;
    op_ = n;
  }
  return op_->v;
}

inline const Value* Value::get(std::string_view k) const {
  if (t != T::Object || !op_) return nullptr;
  for (auto& m : op_->v)
    if (m.k.sv() == k) return &m.v;
  return nullptr;
}
inline const Value* Value::get(const Key& k) const {
  if (t != T::Object || !op_) return nullptr;
  for (auto& m : op_->v)
    if (m.k == k) return &m.v;
  return nullptr;
}
inline Value* Value::get_mut(std::string_view k) {
  if (!get(k)) return nullptr;
  for (auto& m : obj_mut())
    if (m.k.sv() == k) return &m.v;
  return nullptr;
}
inline Value& Value::operator[](std::string_view k) {
  auto& o = obj_mut();
  for (auto& m : o)
    if (m.k.sv() == k) return m.v;
  o.push_back(Member{Key(k), Value()});
  return o.back().v;
}
inline bool Value::erase(std::string_view k) {
  if (!get(k)) return false;
  auto& o = obj_mut();
  for (size_t n = 0; n < o.size(); ++n)
    if (o[n].k.sv() == k) {
      o.erase(o.begin() + n);
      return true;
    }
  return false;
}

inline bool operator==(const Value& a, const Value& b) {
  if (a.t != b.t) {
    if ((a.t == T::Int && b.t == T::Double)) return (double)a.i == b.d;
    if ((a.t == T::Double && b.t == T::Int)) return a.d == (double)b.i;
    return false;
  }
  switch (a.t) {
    case T::Null: return true;
    case T::Bool: return a.b == b.b;
    case T::Int: return a.i == b.i;
    case T::Double: return a.d == b.d;
    case T::String: return a.same(b) || a.s() == b.s();
    case T::Array: {
      if (a.ap_ == b.ap_) return true;
      const auto& x = a.arr();
      const auto& y = b.arr();
      if (x.size() != y.size()) return false;
      for (size_t n = 0; n < x.size(); ++n)
        if (!(x[n] == y[n])) return false;
      return true;
    }
    case T::Object: {
      if (a.op_ == b.op_) return true;
      const auto& x = a.obj();
      const auto& y = b.obj();
      if (x.size() != y.size()) return false;
      for (size_t n = 0; n < x.size(); ++n) {
        // members mostly come in the same order: look there first
        const Value* o = y[n].k == x[n].k ? &y[n].v : b.get(x[n].k);
        if (!o || !(x[n].v == *o)) return false;
      }
      return true;
    }
  }
  return false;
}
inline bool operator!=(const Value& a, const Value& b) { return !(a == b); }

// ------------------------------------------------------------------ parser

class ParseError : public std::runtime_error {
 public:
  using std::runtime_error::runtime_error;
};

// Containers are built in place: the elements of every open container sit on one stack per
// parse, and a container's payload is allocated once, at its closing bracket, at its final size.
class Parser {
 public:
  Parser(const char* p, size_t n) : p_(p), end_(p + n) {
    vals_.reserve(32);
    mems_.reserve(64);
  }
  Value parse() {
    Value v;
    value(0, v);
    ws();
    if (p_ != end_) throw ParseError("trailing characters after JSON value");
    return v;
  }

 private:
  const char* p_;
  const char* end_;
  std::vector<Value> vals_;   // elements of the open arrays, innermost last
  std::vector<Member> mems_;  // members of the open objects
  std::string key_, str_;     // scratch for the key / the string value being read

  void ws() {
    while (p_ < end_ && (*p_ == ' ' || *p_ == '\n' || *p_ == '\r' || *p_ == '\t')) ++p_;
  }
  [[noreturn]] void fail(const char* m) { throw ParseError(m); }

  void value(int depth, Value& out) {
    if (depth > 256) fail("JSON nesting too deep");
    ws();
    if (p_ >= end_) fail("unexpected end of JSON");
    char c = *p_;
    if (c == '{') return object(depth, out);
    if (c == '[') return array(depth, out);
    if (c == '"') {
      str_.clear();
      string(str_);
      out = Value::str(str_);
      return;
    }
    if (c == 't') { lit("true"); out = Value::boolean(true); return; }
    if (c == 'f') { lit("false"); out = Value::boolean(false); return; }
    if (c == 'n') { lit("null"); out = Value(); return; }
    if (c == '-' || (c >= '0' && c <= '9')) return number(out);
    fail("invalid JSON value");
  }
  void lit(const char* w) {
    size_t n = std::strlen(w);
    if ((size_t)(end_ - p_) < n || std::memcmp(p_, w, n) != 0) fail("invalid literal");
    p_ += n;
  }
  void number(Value& out) {
    const char* s = p_;
    bool fl = false;
    if (*p_ == '-') ++p_;
    while (p_ < end_ && ((*p_ >= '0' && *p_ <= '9') || *p_ == '.' || *p_ == 'e' || *p_ == 'E' || *p_ == '+' ||
                         *p_ == '-')) {
      if (*p_ == '.' || *p_ == 'e' || *p_ == 'E') fl = true;
      ++p_;
    }
    if (!fl) {
      int64_t v;
      auto r = std::from_chars(s, p_, v);
      if (r.ec == std::errc() && r.ptr == p_) {
        out = Value::integer(v);
        return;
      }
    }
    double d;
    auto r = std::from_chars(s, p_, d);
    if (r.ec != std::errc() || r.ptr != p_) fail("invalid number");
    out = Value::number(d);
  }
  static void utf8(std::string& out, uint32_t cp) {
    if (cp < 0x80) out += (char)cp;
    else if (cp < 0x800) { out += (char)(0xC0 | (cp >> 6)); out += (char)(0x80 | (cp & 0x3F)); }
    else if (cp < 0x10000) {
      out += (char)(0xE0 | (cp >> 12)); out += (char)(0x80 | ((cp >> 6) & 0x3F)); out += (char)(0x80 | (cp & 0x3F));
    } else {
      out += (char)(0xF0 | (cp >> 18)); out += (char)(0x80 | ((cp >> 12) & 0x3F));
      out += (char)(0x80 | ((cp >> 6) & 0x3F)); out += (char)(0x80 | (cp & 0x3F));
    }
  }
  uint32_t hex4() {
    if (end_ - p_ < 4) fail("bad \\u escape");
    uint32_t v = 0;
    for (int k = 0; k < 4; ++k) {
      char c = *p_++;
      v <<= 4;
      if (c >= '0' && c <= '9') v |= c - '0';
      else if (c >= 'a' && c <= 'f') v |= c - 'a' + 10;
      else if (c >= 'A' && c <= 'F') v |= c - 'A' + 10;
      else fail("bad hex digit");
    }
    return v;
  }
  // the string at p_ (on its opening quote) into `out`, which is empty
  void string(std::string& out) {
    ++p_;  // opening quote
    const char* run = p_;
    while (true) {
      if (p_ >= end_) fail("unterminated string");
      char c = *p_;
      if (c == '"') {
        out.append(run, p_ - run);
        ++p_;
        return;
      }
      if (c == '\\') {
        out.append(run, p_ - run);
        ++p_;
        if (p_ >= end_) fail("bad escape");
        char e = *p_++;
        switch (e) {
          case '"': out += '"'; break;
          case '\\': out += '\\'; break;
          case '/': out += '/'; break;
          case 'b': out += '\b'; break;
          case 'f': out += '\f'; break;
          case 'n': out += '\n'; break;
          case 'r': out += '\r'; break;
          case 't': out += '\t'; break;
          case 'u': {
            uint32_t cp = hex4();
            if (cp >= 0xD800 && cp <= 0xDBFF && end_ - p_ >= 6 && p_[0] == '\\' && p_[1] == 'u') {
              p_ += 2;
              uint32_t lo = hex4();
              if (lo >= 0xDC00 && lo <= 0xDFFF) cp = 0x10000 + ((cp - 0xD800) << 10) + (lo - 0xDC00);
              else { utf8(out, cp); cp = lo; }
            }
            utf8(out, cp);
            break;
          }
          default: fail("bad escape");
        }
        run = p_;
        continue;
      }
      if ((unsigned char)c < 0x20) fail("control character in string");
      ++p_;
    }
  }
  void array(int depth, Value& out) {
    ++p_;
    ws();
    if (p_ < end_ && *p_ == ']') { ++p_; out = Value::array(); return; }
    const size_t base = vals_.size();
    while (true) {
      Value val;
      value(depth + 1, val);
      vals_.push_back(std::move(val));
      ws();
      if (p_ >= end_) fail("unterminated array");
      if (*p_ == ',') { ++p_; continue; }
      if (*p_ == ']') { ++p_; break; }
      fail("expected , or ]");
    }
    out = Value::array_of(std::vector<Value>(std::make_move_iterator(vals_.begin() + base),
                                             std::make_move_iterator(vals_.end())));
    vals_.resize(base);
  }
  void object(int depth, Value& out) {
    ++p_;
    ws();
    if (p_ < end_ && *p_ == '}') { ++p_; out = Value::object(); return; }
    const size_t base = mems_.size();
    while (true) {
      ws();
      if (p_ >= end_ || *p_ != '"') fail("expected object key");
      key_.clear();
      string(key_);
      Key k(key_);  // key_ is reused by the members of the value
      ws();
      if (p_ >= end_ || *p_ != ':') fail("expected :");
      ++p_;
      Value val;
      value(depth + 1, val);
      // duplicate keys: last wins, in the first one's place (encoding/json behaviour)
      size_t n = base;
      while (n < mems_.size() && !(mems_[n].k == k)) ++n;
      if (n < mems_.size()) mems_[n].v = std::move(val);
      else mems_.push_back(Member{std::move(k), std::move(val)});
      ws();
      if (p_ >= end_) fail("unterminated object");
      if (*p_ == ',') { ++p_; continue; }
      if (*p_ == '}') { ++p_; break; }
      fail("expected , or }");
    }
    out = Value::object_of(std::vector<Member>(std::make_move_iterator(mems_.begin() + base),
                                               std::make_move_iterator(mems_.end())));
    mems_.resize(base);
  }
};

inline Value parse(std::string_view s) { return Parser(s.data(), s.size()).parse(); }

// ------------------------------------------------------------------ serializer

inline void escape(std::string& out, std::string_view s) {
  out += '"';
  size_t run = 0;
  for (size_t n = 0; n < s.size(); ++n) {
    unsigned char c = (unsigned char)s[n];
    if (c >= 0x20 && c != '"' && c != '\\') continue;
    const char* rep = nullptr;
    char buf[8];
    if (c == '"') rep = "\\\"";
    else if (c == '\\') rep = "\\\\";
    else if (c == '\n') rep = "\\n";
    else if (c == '\r') rep = "\\r";
    else if (c == '\t') rep = "\\t";
    else {
      std::snprintf(buf, sizeof(buf), "\\u%04x", c);
      rep = buf;
    }
    out.append(s.data() + run, n - run);
    out += rep;
    run = n + 1;
  }
  out.append(s.data() + run, s.size() - run);
  out += '"';
}

inline void dump(std::string& out, const Value& v) {
  switch (v.t) {
    case T::Null: out += "null"; break;
    case T::Bool: out += v.b ? "true" : "false"; break;
    case T::Int: {
      char buf[24];
      auto r = std::to_chars(buf, buf + sizeof(buf), v.i);
      out.append(buf, r.ptr);
      break;
    }
    case T::Double: {
      char buf[32];
      auto r = std::to_chars(buf, buf + sizeof(buf), v.d);
      out.append(buf, r.ptr);
      break;
    }
    case T::String: escape(out, v.s()); break;
    case T::Array: {
      const auto& a = v.arr();
      out += '[';
      for (size_t n = 0; n < a.size(); ++n) {
        if (n) out += ',';
        dump(out, a[n]);
      }
      out += ']';
      break;
    }
    case T::Object: {
      const auto& o = v.obj();
      out += '{';
      for (size_t n = 0; n < o.size(); ++n) {
        if (n) out += ',';
        escape(out, o[n].k.sv());
        out += ':';
        dump(out, o[n].v);
      }
      out += '}';
      break;
    }
  }
}

// The object `v` with its string member `key` written as `val` (appended when `v` has no such
// member): what dump() gives for a copy of `v` with v[key] = val, without the copy.
inline void dump_with(std::string& out, const Value& v, std::string_view key, const std::string& val) {
  if (v.t != T::Object) return dump(out, v);
  const auto& o = v.obj();
  out += '{';
  bool found = false;
  for (size_t n = 0; n < o.size(); ++n) {
    if (n) out += ',';
    escape(out, o[n].k.sv());
    out += ':';
    if (o[n].k == key) {
      found = true;
      escape(out, val);
    } else {
      dump(out, o[n].v);
    }
  }
  if (!found) {
    if (!o.empty()) out += ',';
    escape(out, key);
    out += ':';
    escape(out, val);
  }
  out += '}';
}

inline std::string dump(const Value& v) {
  std::string s;
  s.reserve(512);
  dump(s, v);
  return s;
}

}  // namespace kj
