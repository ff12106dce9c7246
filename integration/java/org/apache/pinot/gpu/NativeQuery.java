/**
 * QueryContext -> the flat little-endian record integration/jni/pinot_gpu_shim.h describes (the native side turns it into a
 * pg_query).  Literals stay strings exactly as the Predicate objects hold them; the native planner parses them against the
 * column's stored type as PredicateEvaluatorProvider does (pinot-core/.../predicate/PredicateEvaluatorProvider.java:45-96).
 * Returns null for query shapes the record cannot express (transform expressions, MV / text / JSON / regexp predicates, other
 * aggregation functions): the plan maker then keeps the default plan.
 */
package org.apache.pinot.gpu;

import java.nio.ByteBuffer;
import java.nio.ByteOrder;
import java.nio.charset.StandardCharsets;
import java.util.List;
import org.apache.commons.lang3.tuple.Pair;
import org.apache.pinot.common.request.context.ExpressionContext;
import org.apache.pinot.common.request.context.FilterContext;
import org.apache.pinot.common.request.context.FunctionContext;
import org.apache.pinot.common.request.context.OrderByExpressionContext;
import org.apache.pinot.common.request.context.predicate.EqPredicate;
import org.apache.pinot.common.request.context.predicate.InPredicate;
import org.apache.pinot.common.request.context.predicate.NotEqPredicate;
import org.apache.pinot.common.request.context.predicate.NotInPredicate;
import org.apache.pinot.common.request.context.predicate.Predicate;
import org.apache.pinot.common.request.context.predicate.RangePredicate;
import org.apache.pinot.core.query.aggregation.function.AggregationFunction;
import org.apache.pinot.core.query.aggregation.function.DistinctCountHLLAggregationFunction;
import org.apache.pinot.core.query.request.context.QueryContext;
import org.apache.pinot.spi.data.FieldSpec;

public final class NativeQuery implements AutoCloseable {
  private static final int MAGIC = 0x32514750;   // "PGQ2": + ORDER BY block, LIMIT, minSegmentGroupTrimSize
  // pg_filter_type / pg_predicate_type / pg_agg_function
  private static final int F_AND = 0, F_OR = 1, F_NOT = 2, F_PREDICATE = 3, F_TRUE = 4, F_FALSE = 5;
  private static final int P_EQ = 0, P_NOT_EQ = 1, P_IN = 2, P_NOT_IN = 3, P_RANGE = 4, P_IS_NULL = 5, P_IS_NOT_NULL = 6;
  private static final int FLAG_SKIP_STAR_TREE = 0x2;
  // PG_QUERY_FLAG_NULL_HANDLING: three-valued filters, null-skipping aggregations, null group keys (pg_query_supported refuses nulls in
  // multi-value columns)
  private static final int FLAG_NULL_HANDLING = 0x40;

  private static final int FLAG_KEEP_DEVICE_TABLE = 0x4;   // PG_QUERY_FLAG_KEEP_DEVICE_TABLE
  private static final int FLAG_DISTINCT = 0x80;          // PG_QUERY_FLAG_DISTINCT
  private static final int FLAG_SELECTION = 0x100;        // PG_QUERY_FLAG_SELECTION

  private final long _address;
  private final int _flags;

  private NativeQuery(long address, int flags) {
    _address = address;
    _flags = flags;
  }

  /** The record asked for the dense accumulator table to stay in HBM with the result (GpuGroupByCombineOperator's library merge). */
  public boolean keepsDeviceTable() {
    return (_flags & FLAG_KEEP_DEVICE_TABLE) != 0;
  }

  public long address() {
    return _address;
  }

  @Override
  public void close() {
    PinotGpu.queryFree(_address);
  }

  public static NativeQuery from(QueryContext q) {
    return from(q, 0);
  }

  /** `extraFlags`: PinotGpu.QUERY_FLAG_* ORed into the record (GpuGroupByCombineOperator asks for QUERY_FLAG_KEEP_DEVICE_TABLE). */
  public static NativeQuery from(QueryContext q, int extraFlags) {
    ByteBuffer b = ByteBuffer.allocateDirect(estimate(q)).order(ByteOrder.LITTLE_ENDIAN);
    List<ExpressionContext> groupBy = q.getGroupByExpressions();
    AggregationFunction[] aggs = q.getAggregationFunctions();
    if (aggs == null || aggs.length == 0) {
      return null;
    }
    // Segment-level group trim (GroupByOperator.java:120-133): the ORDER BY expressions as TableResizer resolves them (TableResizer.java:
    // 129-161) — a group-by expression or an aggregation of the query.  Anything else (post-aggregations, literals, filtered aggregations)
    // leaves the block empty: the segment's groups then come back untrimmed, which only keeps groups the broker would drop anyway.
    int[] orderBy = groupBy == null ? null : orderBy(q, groupBy);
    b.putInt(MAGIC).putInt((q.isSkipStarTree() ? FLAG_SKIP_STAR_TREE : 0) | (q.isNullHandlingEnabled() ? FLAG_NULL_HANDLING : 0) | extraFlags).putInt(q.getNumGroupsLimit())
        .putInt(q.getMaxInitialResultHolderCapacity()).putInt(groupBy == null ? 0 : groupBy.size()).putInt(aggs.length)
        .putInt(q.getFilter() == null ? 0 : 1).putInt(orderBy == null ? 0 : orderBy.length / 4);
    b.putInt(q.getLimit()).putInt(orderBy == null ? -1 : q.getMinSegmentGroupTrimSize());
    if (groupBy != null) {
      for (ExpressionContext e : groupBy) {
        String key = keyText(e);
        if (key == null) {
          return null;
        }
        putString(b, key);
      }
    }
    for (AggregationFunction f : aggs) {
      int fn = function(f);
      List<ExpressionContext> args = f.getInputExpressions();
      if (fn == 21 || fn == 22) {   // PG_AGG_FIRSTWITHTIME / PG_AGG_LASTWITHTIME: the argument list "x,t,'TYPE'" in pg_agg_spec.column
        String list = withTimeArguments(f, args);
        if (list == null) {
          return null;
        }
        b.putInt(fn).putInt(0);
        putString(b, list);
        continue;
      }
      if (fn == 23 || fn == 24) {   // PG_AGG_COVARPOP / PG_AGG_COVARSAMP: the argument list "x,y" in pg_agg_spec.column, two identifiers
        if (args.size() != 2 || args.get(0).getType() != ExpressionContext.Type.IDENTIFIER
            || args.get(1).getType() != ExpressionContext.Type.IDENTIFIER) {
          return null;
        }
        b.putInt(fn).putInt(0);
        putString(b, args.get(0).getIdentifier() + "," + args.get(1).getIdentifier());
        continue;
      }
      if (fn == 27) {   // PG_AGG_HISTOGRAM: the argument list "x,'lower','upper','numBins'" / "x,arrayvalueconstructor(e0,e1,...)" in pg_agg_spec.column
        String list = histogramArguments(q, f);
        if (list == null) {
          return null;
        }
        b.putInt(fn).putInt(0);
        putString(b, list);
        continue;
      }
      if (fn == 28) {   // PG_AGG_MODE: the argument list "x" / "x,'MAX'" in pg_agg_spec.column
        String list = modeArguments(q, f);
        if (list == null) {
          return null;
        }
        b.putInt(fn).putInt(0);
        putString(b, list);
        continue;
      }
      if (fn < 0 || args.size() > 1) {
        return null;
      }
      // the argument: a column, or — for SUM / MIN / MAX / AVG / MINMAXRANGE — an arithmetic expression over columns and literals, with or
      // without a CASE in it, handed over as the text ExpressionContext#toString prints (pg_agg_spec.column; the library parses it, pg_expr.h)
      String argument = args.isEmpty() ? "*" : args.get(0).getType() == ExpressionContext.Type.IDENTIFIER ? args.get(0).getIdentifier()
          : takesExpression(fn) && (isArithmetic(args.get(0)) || isCaseExpression(args.get(0))) ? args.get(0).toString() : null;
      if (argument == null) {
        return null;
      }
      b.putInt(fn).putInt(0);   // log2m 0: DEFAULT_HYPERLOGLOG_LOG2M (a literal second argument is not expressible here)
      putString(b, argument);
      if (fn == 16) {   // PG_AGG_PERCENTILE: its p as one double right after the column (records without a PERCENTILE are unchanged)
        double p = percentileOf(f);
        if (!(p >= 0.0 && p <= 100.0)) {
          return null;
        }
        b.putDouble(p);
      }
    }
    if (orderBy != null) {
      for (int v : orderBy) {
        b.putInt(v);
      }
    }
    if (q.getFilter() != null && !putFilter(b, q.getFilter())) {
      return null;
    }
    return new NativeQuery(PinotGpu.queryParse(b, b.position()), extraFlags);
  }

  /**
   * SELECT DISTINCT (PG_QUERY_FLAG_DISTINCT): the DISTINCT expressions in the group-by slots, no aggregation, every ORDER BY expression a
   * group-key entry, LIMIT always read (Integer.MAX_VALUE: every tuple).  null when an expression is neither a plain column nor an arithmetic
   * expression over columns and literals (the Java plan answers).
   */
  public static NativeQuery fromDistinct(QueryContext q) {
    List<ExpressionContext> columns = q.getSelectExpressions();
    List<OrderByExpressionContext> orderBy = q.getOrderByExpressions();
    int numOrderBy = orderBy == null ? 0 : orderBy.size();
    ByteBuffer b = ByteBuffer.allocateDirect(estimate(q)).order(ByteOrder.LITTLE_ENDIAN);
    b.putInt(MAGIC).putInt(FLAG_DISTINCT | (q.isNullHandlingEnabled() ? FLAG_NULL_HANDLING : 0)).putInt(q.getNumGroupsLimit())
        .putInt(q.getMaxInitialResultHolderCapacity()).putInt(columns.size()).putInt(0)
        .putInt(q.getFilter() == null ? 0 : 1).putInt(numOrderBy);
    b.putInt(q.getLimit()).putInt(-1);
    for (ExpressionContext e : columns) {
      String key = keyText(e);
      if (key == null) {
        return null;
      }
      putString(b, key);
    }
    for (int i = 0; i < numOrderBy; i++) {
      OrderByExpressionContext o = orderBy.get(i);
      int index = columns.indexOf(o.getExpression());
      if (index < 0) {
        return null;
      }
      b.putInt(0).putInt(index).putInt(o.isAsc() ? 1 : 0).putInt(o.isNullsLast() ? 1 : 0);   // PG_ORDER_BY_GROUP_KEY
    }
    if (q.getFilter() != null && !putFilter(b, q.getFilter())) {
      return null;
    }
    return new NativeQuery(PinotGpu.queryParse(b, b.position()), FLAG_DISTINCT);
  }

  /**
   * Selection (PG_QUERY_FLAG_SELECTION): `expressions` (SelectionOperatorUtils#extractExpressions over the segment) in the group-by slots, no
   * aggregation, every ORDER BY expression a group-key entry (none under LIMIT 0), LIMIT the operator's _numRowsToKeep (offset + limit under
   * ORDER BY).  null when an expression is not a plain column (the Java plan answers).
   */
  public static NativeQuery fromSelection(QueryContext q, List<ExpressionContext> expressions) {
    List<OrderByExpressionContext> orderBy = q.getLimit() > 0 ? q.getOrderByExpressions() : null;
    int numOrderBy = orderBy == null ? 0 : orderBy.size();
    int size = estimate(q);
    for (ExpressionContext e : expressions) {
      size += 8 + 4 * e.toString().length();
    }
    ByteBuffer b = ByteBuffer.allocateDirect(size).order(ByteOrder.LITTLE_ENDIAN);
    b.putInt(MAGIC).putInt(FLAG_SELECTION | (q.isNullHandlingEnabled() ? FLAG_NULL_HANDLING : 0)).putInt(q.getNumGroupsLimit())
        .putInt(q.getMaxInitialResultHolderCapacity()).putInt(expressions.size()).putInt(0)
        .putInt(q.getFilter() == null ? 0 : 1).putInt(numOrderBy);
    b.putInt(orderBy == null ? q.getLimit() : q.getOffset() + q.getLimit()).putInt(-1);   // SelectionOrderByOperator._numRowsToKeep
    for (ExpressionContext e : expressions) {
      if (e.getType() != ExpressionContext.Type.IDENTIFIER) {
        return null;
      }
      putString(b, e.getIdentifier());
    }
    for (int i = 0; i < numOrderBy; i++) {
      OrderByExpressionContext o = orderBy.get(i);
      int index = expressions.indexOf(o.getExpression());
      if (index < 0) {
        return null;
      }
      b.putInt(0).putInt(index).putInt(o.isAsc() ? 1 : 0).putInt(o.isNullsLast() ? 1 : 0);   // PG_ORDER_BY_GROUP_KEY
    }
    if (q.getFilter() != null && !putFilter(b, q.getFilter())) {
      return null;
    }
    return new NativeQuery(PinotGpu.queryParse(b, b.position()), FLAG_SELECTION);
  }

  /** {kind, index, ascending, nullsLast} per ORDER BY expression (pg_order_by), or null when the query has none or one the record cannot carry. */
  private static int[] orderBy(QueryContext q, List<ExpressionContext> groupBy) {
    List<OrderByExpressionContext> orderBy = q.getOrderByExpressions();
    if (orderBy == null || orderBy.isEmpty() || q.getMinSegmentGroupTrimSize() <= 0) {
      return null;
    }
    int[] out = new int[4 * orderBy.size()];
    for (int i = 0; i < orderBy.size(); i++) {
      OrderByExpressionContext o = orderBy.get(i);
      ExpressionContext e = o.getExpression();
      int kind;
      int index = groupBy.indexOf(e);
      if (index >= 0) {
        kind = 0;   // PG_ORDER_BY_GROUP_KEY
      } else {
        FunctionContext f = e.getFunction();
        if (f == null || f.getType() != FunctionContext.Type.AGGREGATION) {
          return null;
        }
        Integer a = q.getFilteredAggregationsIndexMap().get(Pair.of(f, null));
        if (a == null) {
          return null;
        }
        kind = 1;   // PG_ORDER_BY_AGGREGATION
        index = a;
      }
      out[4 * i] = kind;
      out[4 * i + 1] = index;
      out[4 * i + 2] = o.isAsc() ? 1 : 0;
      out[4 * i + 3] = o.isNullsLast() ? 1 : 0;
    }
    return out;
  }

  /**
   * The p of an exact PERCENTILE: PercentileAggregationFunction keeps it in a protected field, but names its result column by it —
   * "percentile95(col)" for the legacy form, "percentile(col, 99.9)" otherwise (PercentileAggregationFunction.java:60-64).  NaN when the
   * name has neither shape.  The parse assumes the argument is a plain identifier (no "(" and no ", " inside it), which from() has already
   * checked when it calls this; a column whose name held either would give NaN or a wrong p, so from() refuses anything that is not
   * Type.IDENTIFIER first and an out-of-range or NaN p afterwards.
   */
  static double percentileOf(AggregationFunction f) {
    String name = f.getResultColumnName();
    try {
      int open = name.indexOf('(');
      int comma = name.lastIndexOf(", ");
      if (open > "percentile".length()) {
        return Integer.parseInt(name.substring("percentile".length(), open));
      }
      if (comma > open && name.endsWith(")")) {
        return Double.parseDouble(name.substring(comma + 2, name.length() - 1));
      }
    } catch (NumberFormatException e) {
      return Double.NaN;
    }
    return Double.NaN;
  }

  /** pg_agg_function of a star-tree function-column pair's function type; -1 for functions the GPU path never reads. */
  static int functionCode(org.apache.pinot.segment.spi.AggregationFunctionType type) {
    switch (type) {
      case COUNT: return 0;
      case SUM: return 1;
      case MIN: return 2;
      case MAX: return 3;
      case AVG: return 4;
      case DISTINCTCOUNT: return 5;
      case DISTINCTCOUNTHLL: return 6;
      case MINMAXRANGE: return 7;
      default: return -1;
    }
  }

  /** FIRSTWITHTIME / LASTWITHTIME: the argument list as getResultColumnName prints it between the parentheses — the value column, the time
   *  column (getInputExpressions().get(1)), the declared type quoted; the type comes from the concrete subclass.  Null for an argument that
   *  is no column and for the Boolean / String variants (the Java plan answers). */
  private static String withTimeArguments(AggregationFunction f, List<ExpressionContext> args) {
    String type = withTimeType(f);
    if (type == null || args.size() != 2 || args.get(0).getType() != ExpressionContext.Type.IDENTIFIER
        || args.get(1).getType() != ExpressionContext.Type.IDENTIFIER) {
      return null;
    }
    return args.get(0).getIdentifier() + "," + args.get(1).getIdentifier() + ",'" + type + "'";
  }

  /** HISTOGRAM: the argument list as the query spells it.  The function keeps its bins to itself (no accessor), so they are read where it
   *  read them: the FunctionContext of the query's aggregation with f's result column name — the column, then the three literals or the
   *  arrayvalueconstructor call, each printed by ExpressionContext#toString (a literal quoted, Infinity / -Infinity bare identifiers).  Null
   *  for an argument that is no column, for a filtered aggregation and for a literal array (the Java plan answers). */
  private static String histogramArguments(QueryContext q, AggregationFunction f) {
    for (java.util.Map.Entry<org.apache.commons.lang3.tuple.Pair<org.apache.pinot.common.request.context.FunctionContext,
        org.apache.pinot.common.request.context.FilterContext>, Integer> e : q.getFilteredAggregationsIndexMap().entrySet()) {
      org.apache.pinot.common.request.context.FunctionContext fc = e.getKey().getLeft();
      if (q.getAggregationFunctions()[e.getValue()] != f) {
        continue;
      }
      List<ExpressionContext> args = fc.getArguments();
      if (e.getKey().getRight() != null || (args.size() != 2 && args.size() != 4) || args.get(0).getType() != ExpressionContext.Type.IDENTIFIER) {
        return null;
      }
      StringBuilder list = new StringBuilder(args.get(0).getIdentifier());
      for (int i = 1; i < args.size(); i++) {
        ExpressionContext a = args.get(i);
        boolean array = a.getType() == ExpressionContext.Type.FUNCTION && a.getFunction().getFunctionName().equals("arrayvalueconstructor");
        if (args.size() == 2 ? !array : a.getType() != ExpressionContext.Type.LITERAL) {
          return null;
        }
        list.append(',').append(a.toString());
      }
      return list.toString();
    }
    return null;
  }

  /** MODE: the argument list as the query spells it.  The function keeps its reducer to itself (no accessor), so it is read where the
   *  function read it: the FunctionContext of the query's aggregation — the column, then the MultiModeReducerType literal as
   *  ExpressionContext#toString prints it ('MAX').  Null for an argument that is no column, a filtered aggregation, a second argument that
   *  is no literal, or more than two arguments (the Java plan answers, with the reference's own errors). */
  private static String modeArguments(QueryContext q, AggregationFunction f) {
    for (java.util.Map.Entry<org.apache.commons.lang3.tuple.Pair<org.apache.pinot.common.request.context.FunctionContext,
        org.apache.pinot.common.request.context.FilterContext>, Integer> e : q.getFilteredAggregationsIndexMap().entrySet()) {
      if (q.getAggregationFunctions()[e.getValue()] != f) {
        continue;
      }
      List<ExpressionContext> args = e.getKey().getLeft().getArguments();
      if (e.getKey().getRight() != null || args.isEmpty() || args.size() > 2 || args.get(0).getType() != ExpressionContext.Type.IDENTIFIER) {
        return null;
      }
      if (args.size() == 1) {
        return args.get(0).getIdentifier();
      }
      if (args.get(1).getType() != ExpressionContext.Type.LITERAL) {
        return null;
      }
      return args.get(0).getIdentifier() + "," + args.get(1).toString();
    }
    return null;
  }

  private static String withTimeType(AggregationFunction f) {
    if (f instanceof org.apache.pinot.core.query.aggregation.function.FirstIntValueWithTimeAggregationFunction
        || f instanceof org.apache.pinot.core.query.aggregation.function.LastIntValueWithTimeAggregationFunction) {
      // (a declared BOOLEAN builds the Int class with its boolean flag set: it keeps its own name through getResultColumnName)
      return f.getResultColumnName().toUpperCase().endsWith("'BOOLEAN')") ? null : "INT";
    }
    if (f instanceof org.apache.pinot.core.query.aggregation.function.FirstLongValueWithTimeAggregationFunction
        || f instanceof org.apache.pinot.core.query.aggregation.function.LastLongValueWithTimeAggregationFunction) {
      return "LONG";
    }
    if (f instanceof org.apache.pinot.core.query.aggregation.function.FirstFloatValueWithTimeAggregationFunction
        || f instanceof org.apache.pinot.core.query.aggregation.function.LastFloatValueWithTimeAggregationFunction) {
      return "FLOAT";
    }
    if (f instanceof org.apache.pinot.core.query.aggregation.function.FirstDoubleValueWithTimeAggregationFunction
        || f instanceof org.apache.pinot.core.query.aggregation.function.LastDoubleValueWithTimeAggregationFunction) {
      return "DOUBLE";
    }
    return null;   // FirstStringValueWithTime... / LastStringValueWithTime...
  }

  private static int function(AggregationFunction f) {
    switch (f.getType()) {
      case COUNT: return 0;
      case SUM: return 1;
      case MIN: return 2;
      case MAX: return 3;
      case AVG: return 4;
      case DISTINCTCOUNT: return 5;
      case DISTINCTCOUNTHLL: return f instanceof DistinctCountHLLAggregationFunction ? 6 : -1;
      case MINMAXRANGE: return 7;
      // the multi-value forms (pg_agg_function 8..15): every entry of every matching doc
      case COUNTMV: return 8;
      case SUMMV: return 9;
      case MINMV: return 10;
      case MAXMV: return 11;
      case AVGMV: return 12;
      case MINMAXRANGEMV: return 13;
      case DISTINCTCOUNTMV: return 14;
      case DISTINCTCOUNTHLLMV: return 15;
      // exact PERCENTILE only: the digest-based members of the family (TDigest, KLL, ...) are other types and stay with the Java plan
      case PERCENTILE: return f instanceof org.apache.pinot.core.query.aggregation.function.PercentileAggregationFunction ? 16 : -1;
      // the second-moment statistics (pg_agg_function 17..20): one intermediate (VarianceTuple), four final values
      case VARPOP: return f instanceof org.apache.pinot.core.query.aggregation.function.VarianceAggregationFunction ? 17 : -1;
      case VARSAMP: return f instanceof org.apache.pinot.core.query.aggregation.function.VarianceAggregationFunction ? 18 : -1;
      case STDDEVPOP: return f instanceof org.apache.pinot.core.query.aggregation.function.VarianceAggregationFunction ? 19 : -1;
      case STDDEVSAMP: return f instanceof org.apache.pinot.core.query.aggregation.function.VarianceAggregationFunction ? 20 : -1;
      // the latest / earliest value per key (pg_agg_function 21 / 22): INT / LONG / FLOAT / DOUBLE variants only (withTimeType)
      // the covariances (pg_agg_function 23 / 24): one intermediate (CovarianceTuple), two final values
      case COVARPOP: return f instanceof org.apache.pinot.core.query.aggregation.function.CovarianceAggregationFunction ? 23 : -1;
      case COVARSAMP: return f instanceof org.apache.pinot.core.query.aggregation.function.CovarianceAggregationFunction ? 24 : -1;
      // the third and fourth moments (pg_agg_function 25 / 26): one intermediate (PinotFourthMoment), two final values; the class's third
      // type, FOURTHMOMENT, has no final result and stays with the Java plan
      case SKEWNESS: return f instanceof org.apache.pinot.core.query.aggregation.function.FourthMomentAggregationFunction ? 25 : -1;
      case KURTOSIS: return f instanceof org.apache.pinot.core.query.aggregation.function.FourthMomentAggregationFunction ? 26 : -1;
      // the bin counts (pg_agg_function 27): intermediate and final value the same DoubleArrayList
      // the map value -> count (pg_agg_function 28); the reducer travels in the argument list
      case MODE: return f instanceof org.apache.pinot.core.query.aggregation.function.ModeAggregationFunction ? 28 : -1;
      case HISTOGRAM: return f instanceof org.apache.pinot.core.query.aggregation.function.HistogramAggregationFunction ? 27 : -1;
      case FIRSTWITHTIME:
        return f instanceof org.apache.pinot.core.query.aggregation.function.FirstWithTimeAggregationFunction && withTimeType(f) != null ? 21 : -1;
      case LASTWITHTIME:
        return f instanceof org.apache.pinot.core.query.aggregation.function.LastWithTimeAggregationFunction && withTimeType(f) != null ? 22 : -1;
      default: return -1;
    }
  }

  private static boolean putFilter(ByteBuffer b, FilterContext f) {
    switch (f.getType()) {
      case AND:
      case OR:
      case NOT:
        b.putInt(f.getType() == FilterContext.Type.AND ? F_AND : f.getType() == FilterContext.Type.OR ? F_OR : F_NOT);
        b.putInt(f.getChildren().size());
        for (FilterContext c : f.getChildren()) {
          if (!putFilter(b, c)) {
            return false;
          }
        }
        return true;
      case CONSTANT:
        b.putInt(f.isConstantTrue() ? F_TRUE : F_FALSE).putInt(0);
        return true;
      default:
        return putPredicate(b, f.getPredicate());
    }
  }

  private static boolean putPredicate(ByteBuffer b, Predicate p) {
    // the left-hand side: a column, or an arithmetic expression over columns and literals (ExpressionFilterOperator: WHERE a * b > 10, and
    // every column-to-column comparison, which PredicateComparisonRewriter turns into minus(a,b) > 0) handed over as the text
    // ExpressionContext#toString prints (pg_filter_node.column; the library parses it, as it does an aggregation's argument)
    ExpressionContext lhs = p.getLhs();
    String column = lhs.getType() == ExpressionContext.Type.IDENTIFIER ? lhs.getIdentifier() : isArithmetic(lhs) ? lhs.toString() : null;
    if (column == null) {
      return false;   // another function on the left: the default plan
    }
    b.putInt(F_PREDICATE).putInt(0);
    switch (p.getType()) {
      case EQ:
        header(b, P_EQ, 1, column);
        putString(b, ((EqPredicate) p).getValue());
        bounds(b, null, null, false, false);
        return true;
      case NOT_EQ:
        header(b, P_NOT_EQ, 1, column);
        putString(b, ((NotEqPredicate) p).getValue());
        bounds(b, null, null, false, false);
        return true;
      case IN:
      case NOT_IN: {
        List<String> values = p.getType() == Predicate.Type.IN ? ((InPredicate) p).getValues() : ((NotInPredicate) p).getValues();
        header(b, p.getType() == Predicate.Type.IN ? P_IN : P_NOT_IN, values.size(), column);
        for (String v : values) {
          putString(b, v);
        }
        bounds(b, null, null, false, false);
        return true;
      }
      case RANGE: {
        RangePredicate r = (RangePredicate) p;
        header(b, P_RANGE, 0, column);
        bounds(b, r.getLowerBound(), r.getUpperBound(), r.isLowerInclusive(), r.isUpperInclusive());   // "*" = UNBOUNDED on both sides
        return true;
      }
      case IS_NULL:
      case IS_NOT_NULL:
        header(b, p.getType() == Predicate.Type.IS_NULL ? P_IS_NULL : P_IS_NOT_NULL, 0, column);
        bounds(b, null, null, false, false);
        return true;
      default:
        return false;   // REGEXP_LIKE, TEXT_MATCH, JSON_MATCH, VECTOR_SIMILARITY ...: the default plan
    }
  }

  private static void header(ByteBuffer b, int predicateType, int nValues, String column) {
    b.putInt(predicateType).putInt(nValues);
    putString(b, column);
  }

  private static void bounds(ByteBuffer b, String lower, String upper, boolean lowerInclusive, boolean upperInclusive) {
    putString(b, lower);
    putString(b, upper);
    b.putInt(lowerInclusive ? 1 : 0).putInt(upperInclusive ? 1 : 0);
  }

  private static void putString(ByteBuffer b, String s) {
    if (s == null) {
      b.putInt(-1);
      return;
    }
    byte[] utf8 = s.getBytes(StandardCharsets.UTF_8);
    b.putInt(utf8.length).put(utf8);
    while ((b.position() & 3) != 0) {
      b.put((byte) 0);
    }
  }

  /**
   * A GROUP BY / DISTINCT key as pg_query.group_by_columns carries it: a column's name, or an arithmetic expression or a time-bucket transform
   * as the text ExpressionContext#toString prints (the library groups its DOUBLE / LONG values through a derived key column); null for
   * anything else.
   */
  private static String keyText(ExpressionContext e) {
    return e.getType() == ExpressionContext.Type.IDENTIFIER ? e.getIdentifier() : isArithmetic(e) || isTimeBucket(e) ? e.toString() : null;
  }

  /**
   * A time-bucket transform as a GROUP BY / DISTINCT key (and only there: not an aggregation's argument, a filter's left-hand side or a
   * selection): timeConvert, toEpoch{Seconds,Minutes,Hours,Days}[Rounded|Bucket], dateTimeConvert or dateTrunc over ONE identifier, every
   * other argument a literal.  The library parses the text ExpressionContext#toString prints, groups the transform's LONG values through a
   * derived key column and refuses what it does not run (named time zones, SIMPLE_DATE_FORMAT, WEEKS / MONTHS / YEARS units): the Java plan
   * answers then.
   */
  static boolean isTimeBucket(ExpressionContext e) {
    if (e.getType() != ExpressionContext.Type.FUNCTION || e.getFunction().getType() != FunctionContext.Type.TRANSFORM) {
      return false;
    }
    FunctionContext f = e.getFunction();
    String name = f.getFunctionName();
    boolean family = name.equals("timeconvert") || name.equals("datetimeconvert") || name.equals("datetrunc")
        || name.matches("toepoch(seconds|minutes|hours|days)(rounded|bucket)?");
    if (!family) {
      return false;
    }
    int value = name.equals("datetrunc") ? 1 : 0;
    List<ExpressionContext> args = f.getArguments();
    for (int i = 0; i < args.size(); i++) {
      if (args.get(i).getType() != (i == value ? ExpressionContext.Type.IDENTIFIER : ExpressionContext.Type.LITERAL)) {
        return false;
      }
    }
    return args.size() > value;
  }

  private static boolean takesExpression(int fn) {
    return fn == 1 || fn == 2 || fn == 3 || fn == 4 || fn == 7;   // PG_AGG_SUM, _MIN, _MAX, _AVG, _MINMAXRANGE
  }

  /**
   * A call of add / sub / mult / div or of their aliases plus / minus / times / divide (TransformFunctionType.java:47-50) whose arguments
   * are identifiers, literals or such calls again.  Anything else — another function, a nested aggregation — stays with the Java plan.
   */
  static boolean isArithmetic(ExpressionContext e) {
    if (e.getType() != ExpressionContext.Type.FUNCTION) {
      return false;
    }
    FunctionContext f = e.getFunction();
    if (f.getType() != FunctionContext.Type.TRANSFORM) {
      return false;
    }
    switch (f.getFunctionName()) {
      case "add":
      case "plus":
      case "sub":
      case "minus":
      case "mult":
      case "times":
      case "div":
      case "divide":
        break;
      default:
        return false;
    }
    for (ExpressionContext a : f.getArguments()) {
      if (a.getType() == ExpressionContext.Type.FUNCTION ? !isArithmetic(a)
          : a.getType() != ExpressionContext.Type.IDENTIFIER && a.getType() != ExpressionContext.Type.LITERAL) {
        return false;
      }
    }
    return true;
  }

  /**
   * An expression with a CASE in it (CaseTransformFunction; DESIGN 4.16): calls of the eight arithmetic names, of case, of the six comparisons
   * and of and / or / not, with identifiers or literals as leaves — conditions where a WHEN stands, values everywhere else.  The library parses
   * the text ExpressionContext#toString prints, which shows every literal quoted: it types a literal from its text, as
   * RequestUtils.getLiteral does for a literal the query spells as a number.  Where the two disagree the Java plan answers (false here): a
   * literal whose LiteralContext type is not what its text implies (a number spelled as a string, a CAST folded by the compiler), and a
   * STRING-typed literal compared with a value that can only be numeric.  (A STRING-typed literal against an identifier is the library's to
   * judge: it knows the column's type and refuses a numeric one.)
   */
  static boolean isCaseExpression(ExpressionContext e) {
    return e.getType() == ExpressionContext.Type.FUNCTION && isCaseValue(e) && !isArithmetic(e);
  }

  private static boolean isCaseValue(ExpressionContext e) {
    if (e.getType() == ExpressionContext.Type.IDENTIFIER) {
      return true;
    }
    if (e.getType() == ExpressionContext.Type.LITERAL) {
      return impliedType(e) != FieldSpec.DataType.STRING && e.getLiteral().getType() == impliedType(e);
    }
    if (e.getType() != ExpressionContext.Type.FUNCTION || e.getFunction().getType() != FunctionContext.Type.TRANSFORM) {
      return false;
    }
    FunctionContext f = e.getFunction();
    List<ExpressionContext> args = f.getArguments();
    switch (f.getFunctionName()) {
      case "add":
      case "plus":
      case "sub":
      case "minus":
      case "mult":
      case "times":
      case "div":
      case "divide":
        for (ExpressionContext a : args) {
          if (!isCaseValue(a)) {
            return false;
          }
        }
        return true;
      case "case":
        if (args.size() < 3 || args.size() % 2 == 0) {
          return false;
        }
        for (int i = 0; i + 1 < args.size(); i += 2) {
          if (!isCaseCondition(args.get(i)) || !isCaseValue(args.get(i + 1))) {
            return false;
          }
        }
        ExpressionContext otherwise = args.get(args.size() - 1);   // an omitted ELSE and ELSE NULL: the literal 'null'
        boolean none = otherwise.getType() == ExpressionContext.Type.LITERAL
            && (otherwise.getLiteral().isNull() || "null".equals(otherwise.getLiteral().getStringValue()));
        return none || isCaseValue(otherwise);
      default:
        return false;
    }
  }

  private static boolean isCaseCondition(ExpressionContext e) {
    if (e.getType() != ExpressionContext.Type.FUNCTION || e.getFunction().getType() != FunctionContext.Type.TRANSFORM) {
      return false;
    }
    FunctionContext f = e.getFunction();
    List<ExpressionContext> args = f.getArguments();
    switch (f.getFunctionName()) {
      case "and":
      case "or":
      case "not":
        for (ExpressionContext a : args) {
          if (!isCaseCondition(a)) {
            return false;
          }
        }
        return f.getFunctionName().equals("not") ? args.size() == 1 : args.size() >= 2;
      case "equals":
      case "notequals":
        if (args.size() != 2) {
          return false;
        }
        for (int i = 0; i < 2; i++) {   // a string literal: against an identifier only, and typed STRING
          ExpressionContext a = args.get(i);
          if (a.getType() == ExpressionContext.Type.LITERAL && impliedType(a) == FieldSpec.DataType.STRING) {
            return a.getLiteral().getType() == FieldSpec.DataType.STRING && args.get(1 - i).getType() == ExpressionContext.Type.IDENTIFIER;
          }
        }
        return isCaseValue(args.get(0)) && isCaseValue(args.get(1));
      case "greaterthan":
      case "greaterthanorequal":
      case "lessthan":
      case "lessthanorequal":
        return args.size() == 2 && isCaseValue(args.get(0)) && isCaseValue(args.get(1));
      default:
        return false;
    }
  }

  /** The type RequestUtils.getLiteral gives a literal spelled as this one's text: INT, LONG, DOUBLE — or STRING when it is no number. */
  private static FieldSpec.DataType impliedType(ExpressionContext literal) {
    String text = literal.getLiteral().getStringValue();
    try {
      Integer.parseInt(text);
      return FieldSpec.DataType.INT;
    } catch (NumberFormatException notAnInt) {
      try {
        Long.parseLong(text);
        return FieldSpec.DataType.LONG;
      } catch (NumberFormatException notALong) {
        try {
          Double.parseDouble(text);
          return FieldSpec.DataType.DOUBLE;
        } catch (NumberFormatException notANumber) {
          return FieldSpec.DataType.STRING;
        }
      }
    }
  }

  private static int estimate(QueryContext q) {
    return 4096 + 64 * q.toString().length();
  }
}
