// Arithmetic expressions as GROUP BY / DISTINCT keys: `group_by_columns[j]` may spell add / sub / mult / div over single-value
// numeric columns and literals, under the rules of pg_agg_spec.column (pg_expr.h).  The reference groups a transform's DOUBLE result through the
// no-dictionary key generators; here the expression becomes a DERIVED column — DOUBLE, no dictionary, no forward index, only a virtual
// dictionary (pg_vdict.hip) whose keys pg_expr_keys computed — and from there on it is a raw DOUBLE key column to every group-by, DISTINCT,
// trim and side-pass kernel.
//
// Derived columns are cached per segment by text (Segment::derived_keys, at most PG_MAX_DERIVED_KEYS, least recently used first out) and
// shared-owned.  Locking follows the bounds pass of expressions inside aggregations and the filter leaves: checks and refusals under seg.mu,
// the full-segment passes (key kernel, sort) outside it, insertion under it again; two threads that meet on a new text may both build, the
// first insertion stays.
#include "pg_internal.hpp"
#include "pg_expr.h"
#include "pg_time_expr.h"

#include <algorithm>

namespace pg {
namespace {

struct Held {
  Segment* seg;
  std::shared_ptr<Column> col;
};
// the derived columns of the queries the calling thread is planning or running, innermost scope last
thread_local std::vector<Held> t_held;

std::string short_text(const std::string& t) { return t.size() > 200 ? t.substr(0, 197) + "..." : t; }

struct KeySpec {
  std::string text;
  bool time = false;     // a time-bucket transform: `targs`, a LONG column; else `args`, a DOUBLE column
  PgExprArgs args;
  PgTimeKeyArgs targs;
  std::vector<Column*> cols;
};

// the value column of a time-bucket transform, checked (seg.mu held): a single-value INT / LONG column, dictionary-encoded or raw
Column* time_value_column(Segment& seg, const std::string& name, bool null_handling) {
  Column* c = seg.find(name.c_str());
  if (!c) fail(PG_ERR_NOT_FOUND, "column not found: %s", short_text(name).c_str());
  if (c->is_mv || c->raw_mv) fail(PG_ERR_UNSUPPORTED, "time function over the multi-value column %s", c->name.c_str());
  if (c->data_type != PG_TYPE_INT && c->data_type != PG_TYPE_LONG)
    fail(PG_ERR_UNSUPPORTED, "time function over the %s column %s (INT and LONG value columns run on the GPU path)",
         c->data_type == PG_TYPE_FLOAT ? "FLOAT" : c->data_type == PG_TYPE_DOUBLE ? "DOUBLE" : c->data_type == PG_TYPE_STRING ? "STRING" : "BYTES", c->name.c_str());
  return expr_operand_column(seg, name, null_handling);   // nulls and layout: the rules and texts every expression shares (pg_plan.cpp)
}

// one expression key, checked and resolved (seg.mu held): the program and its operand columns
KeySpec key_spec(Segment& seg, const char* text, bool null_handling) {
  KeySpec K;
  K.text = text;
  memset(&K.args, 0, sizeof(K.args));
  memset(&K.targs, 0, sizeof(K.targs));
  std::string error;
  if (time_expr_is_time_function(text)) {   // by function name, before the arithmetic parser (which knows none of them)
    TimeProgram tp;
    const int32_t st = time_expr_parse(text, tp, error);
    if (st != PG_OK) fail(st, "%s (in %s)", error.c_str(), short_text(K.text).c_str());
    Column* c = time_value_column(seg, tp.column, null_handling);
    K.time = true;
    expr_fill_src(K.targs.src, *c);
    K.targs.n_docs = seg.total_docs;
    K.targs.n_words = ((int64_t)seg.total_docs + 63) / 64;
    K.targs.prog = tp.prog;
    K.cols.push_back(c);
    return K;
  }
  ExprProgram prog;
  const int32_t st = expr_parse(text, prog, error);
  if (st != PG_OK) fail(st, "%s (in %s)", error.c_str(), short_text(K.text).c_str());
  if (prog.conditional)   // (its type would be the branches' — INT, LONG ... —, not the DOUBLE of the derived key column)
    fail(PG_ERR_UNSUPPORTED, "a CASE, a comparison or a logical call as a GROUP BY / DISTINCT key (%s): inside SUM, MIN, MAX, AVG and MINMAXRANGE they run on the GPU path", short_text(K.text).c_str());
  for (const std::string& name : prog.columns) {
    Column* c = expr_operand_column(seg, name, null_handling);   // the rules every expression shares (pg_plan.cpp)
    expr_fill_src(K.args.srcs[K.cols.size()], *c);               // (expr_parse admits at most PG_EXPR_MAX_SRCS columns)
    K.cols.push_back(c);
  }
  K.args.scan.n_docs = seg.total_docs;
  K.args.scan.n_words = ((int64_t)seg.total_docs + 63) / 64;
  K.args.n_srcs = (int32_t)K.cols.size();
  K.args.n_exprs = 1;
  K.args.count_slot = -1;
  K.args.exprs[0].first_step = 0;
  K.args.exprs[0].n_steps = prog.n_steps;
  for (int k = 0; k < prog.n_steps; k++) K.args.steps[k] = prog.steps[k];
  return K;
}

// the derived column of K: one pass of pg_expr_keys / pg_time_keys and the virtual dictionary's build (seg.mu NOT held)
std::shared_ptr<Column> build_column(Segment& seg, const KeySpec& K, uint64_t* bytes) {
  auto col = std::make_shared<Column>();
  col->name = K.text;
  col->data_type = K.time ? PG_TYPE_LONG : PG_TYPE_DOUBLE;
  col->has_dictionary = false;
  col->col_kind = PG_COL_RAW64;
  col->val_type = K.time ? PG_V_I64 : PG_V_F64;
  col->expr_operands = K.cols;
  col->vdict = K.time ? time_virtual_dictionary(seg, K.text, K.targs, bytes) : expression_virtual_dictionary(seg, K.text, K.args, bytes);
  return col;
}

}  // namespace

ExprKeyScope::ExprKeyScope(Segment& seg, const pg_query& q) : mark_(t_held.size()) {
  if (q.flags & PG_QUERY_FLAG_SELECTION) return;   // selection_shape refuses an expression among the output columns
  if (q.n_group_by <= 0 || !q.group_by_columns) return;
  std::vector<const char*> texts;
  for (int j = 0; j < q.n_group_by; j++) {
    const char* t = q.group_by_columns[j];
    if (!expr_is_expression(t)) continue;
    bool seen = false;
    for (const char* u : texts) seen = seen || !strcmp(u, t);
    if (!seen) texts.push_back(t);
  }
  if (texts.empty()) return;
  if (texts.size() > PG_MAX_EXPR_KEYS)
    fail(PG_ERR_UNSUPPORTED, "more than %d expressions among the group-by / DISTINCT keys of one query", PG_MAX_EXPR_KEYS);
  const bool null_handling = (q.flags & PG_QUERY_FLAG_NULL_HANDLING) != 0;
  std::vector<KeySpec> build;
  std::vector<std::shared_ptr<Column>> mine;
  std::unique_lock<std::mutex> lock(seg.mu);
  for (int j = 0; j < q.n_group_by; j++) {
    const char* t = q.group_by_columns[j];
    if (expr_is_expression(t)) continue;
    Column* c = t ? seg.find(t) : nullptr;
    if (c && (c->is_mv || c->raw_mv))
      fail(PG_ERR_UNSUPPORTED, "the multi-value group-by column %s next to the expression key %s", c->name.c_str(), short_text(texts[0]).c_str());
  }
  for (const char* t : texts) {
    auto it = seg.derived_keys.find(t);
    if (it == seg.derived_keys.end()) {
      build.push_back(key_spec(seg, t, null_handling));
      continue;
    }
    // a column another query built: what depends on the query is checked again
    if (null_handling)
      for (Column* c : it->second.col->expr_operands)
        if (column_has_nulls(seg, c->name)) fail(PG_ERR_UNSUPPORTED, "enableNullHandling: expression over %s, which holds nulls", c->name.c_str());
    it->second.last_used = ++seg.derived_clock;
    mine.push_back(it->second.col);
  }
  if (!build.empty()) {
    lock.unlock();
    std::vector<std::shared_ptr<Column>> built;
    std::vector<uint64_t> bytes(build.size(), 0);
    for (size_t i = 0; i < build.size(); i++) built.push_back(build_column(seg, build[i], &bytes[i]));
    lock.lock();
    for (size_t i = 0; i < build.size(); i++) {
      auto it = seg.derived_keys.find(build[i].text);
      if (it == seg.derived_keys.end()) {
        while (seg.derived_keys.size() >= PG_MAX_DERIVED_KEYS) {
          auto victim = seg.derived_keys.begin();
          for (auto v = seg.derived_keys.begin(); v != seg.derived_keys.end(); ++v)
            if (v->second.last_used < victim->second.last_used) victim = v;
          seg.device_bytes -= std::min(seg.device_bytes, victim->second.bytes);
          seg.derived_keys.erase(victim);   // plans compiled against it keep it alive
        }
        Segment::DerivedKey d;
        d.col = built[i];
        d.bytes = bytes[i];
        seg.device_bytes += bytes[i];
        it = seg.derived_keys.emplace(build[i].text, std::move(d)).first;
      }
      it->second.last_used = ++seg.derived_clock;
      mine.push_back(it->second.col);
    }
  }
  for (auto& c : mine) t_held.push_back({&seg, std::move(c)});
}

ExprKeyScope::~ExprKeyScope() {
  if (t_held.size() > mark_) t_held.resize(mark_);
}

Column* group_key_column(Segment& seg, const char* text, std::shared_ptr<Column>* keep) {
  if (!expr_is_expression(text)) return text ? seg.find(text) : nullptr;
  // the calling thread's own first: the segment's cache may have dropped the column since the scope was opened
  for (auto h = t_held.rbegin(); h != t_held.rend(); ++h)
    if (h->seg == &seg && h->col->name == text) {
      if (keep) *keep = h->col;
      return h->col.get();
    }
  auto it = seg.derived_keys.find(text);
  if (it == seg.derived_keys.end())
    fail(PG_ERR_INTERNAL, "the key column of the expression %s was not prepared before the query was planned", short_text(text).c_str());
  it->second.last_used = ++seg.derived_clock;
  if (keep) *keep = it->second.col;
  return it->second.col.get();
}

}  // namespace pg
