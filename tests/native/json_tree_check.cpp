// Stand-alone check of the apiserver's copy-on-write JSON tree (json.hpp): built and run by
// tests/test_json_tree.py, plain and under the sanitizers.  Exits 0 and prints "OK <n> checks",
// or prints every failed check and exits 1.
#include <atomic>
#include <cstdio>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "json.hpp"

using kj::T;
using kj::Value;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond, what)                                                          \
  do {                                                                             \
    ++g_checks;                                                                    \
    if (!(cond)) {                                                                 \
      ++g_failed;                                                                  \
      std::printf("FAIL %s:%d %s [%s]\n", __FILE__, __LINE__, #cond, std::string(what).c_str()); \
    }                                                                              \
  } while (0)

// node-by-node comparison written against the const views only (no operator==, no identity):
// numbers compare across int / double as operator== documents, objects in any member order
static bool slow_equal(const Value& a, const Value& b) {
  if (a.t != b.t) {
    if (a.t == T::Int && b.t == T::Double) return (double)a.i == b.d;
    if (a.t == T::Double && b.t == T::Int) return a.d == (double)b.i;
    return false;
  }
  switch (a.t) {
    case T::Null: return true;
    case T::Bool: return a.b == b.b;
    case T::Int: return a.i == b.i;
    case T::Double: return a.d == b.d;
    case T::String: return a.s() == b.s();
    case T::Array:
      if (a.arr().size() != b.arr().size()) return false;
      for (size_t n = 0; n < a.arr().size(); ++n)
        if (!slow_equal(a.arr()[n], b.arr()[n])) return false;
      return true;
    case T::Object:
      if (a.obj().size() != b.obj().size()) return false;
      for (auto& m : a.obj()) {
        const Value* o = nullptr;
        for (auto& x : b.obj())
          if (x.k.sv() == m.k.sv()) o = &x.v;
        if (!o || !slow_equal(m.v, *o)) return false;
      }
      return true;
  }
  return false;
}

// every container in `v`, as the chain of steps from the root (object key or array index)
struct Step {
  bool idx;
  std::string key;
  size_t n;
};
using Path = std::vector<Step>;
static void containers(const Value& v, Path& at, std::vector<Path>& out) {
  if (v.is_obj()) {
    out.push_back(at);
    for (auto& m : v.obj()) {
      at.push_back({false, m.k.str(), 0});
      containers(m.v, at, out);
      at.pop_back();
    }
  } else if (v.is_arr()) {
    out.push_back(at);
    for (size_t n = 0; n < v.arr().size(); ++n) {
      at.push_back({true, "", n});
      containers(v.arr()[n], at, out);
      at.pop_back();
    }
  }
}
// the value at `p` for writing: each level on the way is detached, as a patch does it
static Value* descend(Value& root, const Path& p) {
  Value* cur = &root;
  for (auto& s : p) cur = s.idx ? &cur->arr_mut()[s.n] : cur->get_mut(s.key);
  return cur;
}
static const Value* look(const Value& root, const Path& p) {
  const Value* cur = &root;
  for (auto& s : p) cur = s.idx ? &cur->arr()[s.n] : cur->get(s.key);
  return cur;
}

// every mutator at the container `p` of a copy of `orig`; the original must not move, and the
// copy must hold exactly the edit (compared with the same edit made on a separately parsed tree)
static void mutate_everywhere(const std::string& text, const std::string& label) {
  const Value orig = kj::parse(text);
  const std::string before = kj::dump(orig);
  std::vector<Path> where;
  Path at;
  containers(orig, at, where);
  // the edits, each applied to the container it is given
  std::vector<std::pair<std::string, std::function<void(Value&)>>> edits = {
      {"insert", [](Value& c) { if (c.is_obj()) c["added-by-the-check"] = Value::integer(7); else c.arr_mut().push_back(Value::integer(7)); }},
      {"insert-short", [](Value& c) { if (c.is_obj()) c["z"] = Value::str("v"); else c.arr_mut().insert(c.arr_mut().begin(), Value::str("v")); }},
      {"erase-first", [](Value& c) {
         if (c.is_obj()) { if (!c.obj().empty()) c.erase(c.obj()[0].k.str()); }
         else if (!c.arr().empty()) c.arr_mut().erase(c.arr_mut().begin());
       }},
      {"replace-first", [](Value& c) {
         if (c.is_obj()) { if (!c.obj().empty()) c[c.obj()[0].k.str()] = Value::boolean(true); }
         else if (!c.arr().empty()) c.arr_mut()[0] = Value::boolean(true);
       }},
      {"replace-last-member", [](Value& c) { if (c.is_obj() && !c.obj().empty()) c.obj_mut().back().v = Value::number(0.5); }},
      {"get_mut", [](Value& c) {
         if (c.is_obj() && !c.obj().empty()) *c.get_mut(c.obj()[0].k.str()) = Value::null();
       }},
      {"erase-absent", [](Value& c) { if (c.is_obj()) c.erase("not-a-member-of-anything"); }},
  };
  for (auto& p : where)
    for (auto& e : edits) {
      Value copy = orig;
      CHECK(copy.same(orig), label + " copy shares the root");
      e.second(*descend(copy, p));
      CHECK(kj::dump(orig) == before, label + " original unchanged after " + e.first);
      Value fresh = kj::parse(text);  // nothing shared with anything
      e.second(*descend(fresh, p));
      CHECK(kj::dump(copy) == kj::dump(fresh), label + " copy holds exactly the edit " + e.first);
      CHECK((copy == fresh) && slow_equal(copy, fresh), label + " == after " + e.first);
      CHECK((copy == orig) == slow_equal(copy, orig), label + " == against the original after " + e.first);
      // what the edit did not touch is still shared with the original: siblings of the path
      if (!p.empty() && e.first == "insert") {
        const Path parent(p.begin(), p.end() - 1);
        const Value* po = look(orig, parent);
        const Value* pc = look(copy, parent);
        if (po->is_obj())
          for (auto& m : po->obj())
            if (m.k.sv() != p.back().key || p.back().idx) CHECK(pc->get(m.k)->same(m.v), label + " sibling still shared");
      }
    }
}

static void roundtrip(const std::string& text, const std::string& label) {
  Value v = kj::parse(text);
  CHECK(kj::dump(v) == text, label + " parse then dump is the input");
  Value w = kj::parse(text);
  CHECK(v == w, label + " separately parsed trees are equal");
  CHECK(slow_equal(v, w), label + " node by node too");
  Value c = v;
  CHECK(c == v && slow_equal(c, v), label + " a copy is equal");
}

static bool refuses(const std::string& text) {
  try {
    kj::parse(text);
  } catch (const kj::ParseError&) {
    return true;
  }
  return false;
}

int main() {
  const size_t keys_at_start = kj::detail::keys_interned();
  {
    // ---- the cases: objects of 0, 1, 2 members; three deep; array of objects; keys of 15 and
    // 16 bytes (the last inline key, the first interned one); strings of 14 and 15 bytes (the last
    // in the value, the first behind a payload); every escape and a surrogate pair
    const std::vector<std::pair<std::string, std::string>> cases = {
        {"empty", "{}"},
        {"one", "{\"a\":1}"},
        {"two", "{\"b\":\"x\",\"a\":[1,2.5,null,true,false]}"},
        {"deep", "{\"l1\":{\"l2\":{\"l3\":{\"leaf\":\"v\",\"n\":-3}},\"s\":\"t\"},\"tail\":[]}"},
        {"array-of-objects", "[{\"name\":\"a\",\"v\":1},{\"name\":\"b\",\"v\":{\"w\":[{}]}},{}]"},
        {"keys-15-16", "{\"fifteen-bytes-k\":1,\"sixteen-bytes-ke\":2,\"fifteen-bytes-k2\":{\"sixteen-bytes-ke\":[\"x\"]}}"},
        {"strings-14-15", "{\"in\":\"fourteen-bytes\",\"out\":\"fifteen-bytes!!\",\"l\":[\"fourteen-bytes\",\"fifteen-bytes!!\",\"\"]}"},
        {"escapes", "{\"e\":\"q\\\" b\\\\ nl\\n cr\\r tab\\t u\\u0001\\u001f \xF0\x9F\x98\x80 /\"}"},
        {"numbers", "[0,-1,9223372036854775807,1.5,1e+30,0.1,-2.5e-07]"},
    };
    for (auto& c : cases) {
      roundtrip(c.second, c.first);
      mutate_everywhere(c.second, c.first);
    }
    CHECK(kj::parse("{\"fifteen-bytes-k\":1}").obj()[0].k.size() == 15, "15-byte key");
    CHECK(kj::parse("{\"sixteen-bytes-ke\":1}").obj()[0].k.size() == 16, "16-byte key");
    // a string of 14 bytes is the last that lives in the value, one of 15 the first behind a payload
    {
      Value in = kj::parse("\"fourteen-bytes\""), out = kj::parse("\"fifteen-bytes!!\"");
      CHECK(in.s().size() == 14 && out.s().size() == 15, "string lengths");
      CHECK(in.same(kj::parse("\"fourteen-bytes\"")), "equal short strings are the same bits");
      CHECK(!out.same(kj::parse("\"fifteen-bytes!!\"")) && out == kj::parse("\"fifteen-bytes!!\""), "equal long strings compare by bytes");
      Value c = out;
      CHECK(c.same(out) && c.s().data() == out.s().data(), "a copied long string shares its bytes");
      Value m = std::move(in);
      CHECK(m.s() == "fourteen-bytes" && in.is_null(), "a moved short string takes its bytes along");
    }

    // ---- what the escapes decode to, and what dump writes for them
    {
      Value v = kj::parse("\"\\u0041\\b\\f\\/\\ud83d\\ude00\\u00e9\"");
      CHECK(v.s() == std::string("A\b\f/\xF0\x9F\x98\x80\xC3\xA9"), "escapes decoded");
      CHECK(kj::dump(v) == "\"A\\u0008\\u000c/\xF0\x9F\x98\x80\xC3\xA9\"", "escapes written");
      Value lone = kj::parse("\"\\ud83dx\"");  // a lone high surrogate is kept as it came
      CHECK(lone.s() == std::string("\xED\xA0\xBDx"), "lone surrogate");
      Value pair2 = kj::parse("\"\\ud83d\\u0041\"");  // high surrogate, then a non-surrogate escape
      CHECK(pair2.s() == std::string("\xED\xA0\xBD") + "A", "surrogate then plain escape");
    }
    // ---- strictness
    CHECK(refuses("{\"a\":1,}"), "trailing comma");
    CHECK(refuses("{\"a\":\"\x01\"}"), "control character");
    CHECK(refuses("[1] x"), "trailing characters");
    CHECK(refuses("{\"a\":\"\\x\"}"), "bad escape");
    CHECK(refuses(std::string(258, '[') + std::string(258, ']')), "depth limit");
    CHECK(!refuses(std::string(256, '[') + std::string(256, ']')), "depth below the limit");
    CHECK(kj::parse("1").t == T::Int && kj::parse("1.0").t == T::Double && kj::parse("1e2").t == T::Double, "int / double split");
    CHECK(kj::parse("9223372036854775808").t == T::Double, "an integer past int64 is a double");
    CHECK(kj::parse("1") == kj::parse("1.0"), "1 == 1.0");

    // ---- a duplicated key: the last value, in the first one's place
    {
      Value v = kj::parse("{\"a\":1,\"b\":2,\"a\":{\"x\":3},\"sixteen-bytes-ke\":4,\"sixteen-bytes-ke\":5}");
      CHECK(kj::dump(v) == "{\"a\":{\"x\":3},\"b\":2,\"sixteen-bytes-ke\":5}", "duplicate key: last wins");
    }
    // ---- object equality ignores member order; dump keeps it
    {
      Value a = kj::parse("{\"x\":1,\"y\":{\"p\":[1],\"q\":2}}");
      Value b = kj::parse("{\"y\":{\"q\":2,\"p\":[1]},\"x\":1}");
      CHECK(a == b && slow_equal(a, b), "member order does not matter to ==");
      CHECK(kj::dump(a) != kj::dump(b), "but is kept by dump");
      Value c = kj::parse("{\"y\":{\"q\":2,\"p\":[2]},\"x\":1}");
      CHECK(!(a == c) && !slow_equal(a, c), "a difference three deep is found");
    }
    // ---- dump_with
    {
      Value v = kj::parse("{\"apiVersion\":\"g/v1\",\"kind\":\"K\"}");
      std::string out;
      kj::dump_with(out, v, "apiVersion", "g/v2");
      CHECK(out == "{\"apiVersion\":\"g/v2\",\"kind\":\"K\"}", "dump_with replaces");
      out.clear();
      kj::dump_with(out, kj::parse("{\"kind\":\"K\"}"), "apiVersion", "g/v2");
      CHECK(out == "{\"kind\":\"K\",\"apiVersion\":\"g/v2\"}", "dump_with appends");
      out.clear();
      kj::dump_with(out, kj::parse("{}"), "apiVersion", "g/v2");
      CHECK(out == "{\"apiVersion\":\"g/v2\"}", "dump_with into the empty object");
    }
    // ---- one subtree at two positions of a second tree
    {
      Value sub = kj::parse("{\"sixteen-bytes-ke\":[{\"n\":1}],\"s\":\"shared\"}");
      const std::string sub_text = kj::dump(sub);
      Value host = kj::parse("{\"first\":null,\"list\":[0,null]}");
      host["first"] = sub;
      host.get_mut("list")->arr_mut()[1] = sub;
      CHECK(host.get("first")->same(sub) && host.get("list")->arr()[1].same(sub), "both places share the payload");
      CHECK(*host.get("first") == host.get("list")->arr()[1], "== by identity");
      CHECK(kj::dump(host) == "{\"first\":" + sub_text + ",\"list\":[0," + sub_text + "]}", "dumped at both places");
      // an edit through one position stays there
      (*host.get_mut("first"))["s"] = Value::str("edited");
      CHECK(kj::dump(sub) == sub_text, "the subtree itself is unchanged");
      CHECK(kj::dump(host.get("list")->arr()[1]) == sub_text, "and so is its other position");
      CHECK(host.get("first")->sv("s") == "edited", "the edit is where it was made");
      CHECK(!(*host.get("first") == host.get("list")->arr()[1]), "no longer equal");
      CHECK(host.get("first")->get("sixteen-bytes-ke")->same(*sub.get("sixteen-bytes-ke")), "the untouched member is still shared");
      // three deep through the shared subtree
      host.get_mut("list")->arr_mut()[1].get_mut("sixteen-bytes-ke")->arr_mut()[0]["n"] = Value::integer(2);
      CHECK(kj::dump(sub) == sub_text, "unchanged after a deep edit through the other position");
      CHECK(kj::dump(*host.get("first")->get("sixteen-bytes-ke")) == "[{\"n\":1}]", "the first position kept the old leaf");
    }
    // ---- threads: eight copy one shared tree and edit their copies, two dump the shared one
    {
      const Value shared = kj::parse(
          "{\"metadata\":{\"name\":\"n\",\"labels\":{\"a\":\"1\",\"a-label-key-longer-than-fifteen\":\"2\"}},"
          "\"spec\":{\"list\":[{\"name\":\"c\",\"env\":[{\"name\":\"E\",\"value\":\"v\"}]}]},\"status\":{\"n\":0}}");
      const std::string want = kj::dump(shared);
      std::atomic<bool> stop{false};
      std::atomic<int> bad{0};
      std::vector<std::thread> ts;
      for (int d = 0; d < 2; ++d)
        ts.emplace_back([&] {
          while (!stop.load())
            if (kj::dump(shared) != want) bad++;
        });
      std::vector<std::thread> ed;
      for (int w = 0; w < 8; ++w)
        ed.emplace_back([&, w] {
          for (int round = 0; round < 300; ++round) {
            Value mine = shared;
            mine["status"]["n"] = Value::integer(w * 1000 + round);
            (*mine.get_mut("metadata"))["labels"]["a-key-made-by-writer-" + std::to_string(w)] = Value::str("x");
            mine.get_mut("spec")->get_mut("list")->arr_mut()[0].get_mut("env")->arr_mut().push_back(Value::integer(round));
            mine.get_mut("metadata")->get_mut("labels")->erase("a");
            if (mine.get("status")->get("n")->i != w * 1000 + round) bad++;
            if (mine.get("spec")->get("list")->arr()[0].get("env")->arr().size() != 2) bad++;
            if (mine.get("metadata")->get("labels")->get("a")) bad++;
            if (!(mine.get("spec")->get("list")->arr()[0].get("name")->same(*shared.get("spec")->get("list")->arr()[0].get("name")))) bad++;
          }
        });
      for (auto& t : ed) t.join();
      stop = true;
      for (auto& t : ts) t.join();
      CHECK(bad.load() == 0, "threads: private edits stay private");
      CHECK(kj::dump(shared) == want, "threads: the shared tree never changed");
    }
  }
  // every tree is gone: the key table holds nothing of theirs (it counts references per key)
  CHECK(kj::detail::keys_interned() == keys_at_start, "no interned key outlives its trees");
  CHECK(keys_at_start == 0, "nothing interned before the first parse");

  if (g_failed) {
    std::printf("%d of %d checks failed\n", g_failed, g_checks);
    return 1;
  }
  std::printf("OK %d checks\n", g_checks);
  return 0;
}
