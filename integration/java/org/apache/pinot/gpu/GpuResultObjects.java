/**
 * Native result arrays -> the intermediate-result OBJECTS the reference's combine / reduce stages expect:
 *
 *   DISTINCTCOUNT      per group the dictIds of the group's set (pg_result_set_sizes / _set_dict_ids) -> the typed value Set
 *                      BaseDistinctAggregateAggregationFunction#extractGroupByResult builds from its dictId bitmap
 *                      (pinot-core/.../aggregation/function/BaseDistinctAggregateAggregationFunction.java:306-345,646-665,760-806:
 *                      IntOpenHashSet / LongOpenHashSet / FloatOpenHashSet / DoubleOpenHashSet / ObjectOpenHashSet by stored type,
 *                      BYTES wrapped in ByteArray)
 *   DISTINCTCOUNTHLL   per group 2^log2m one-byte registers (pg_result_hll_registers) -> com.clearspring.analytics HyperLogLog over a
 *                      RegisterSet whose int[] packs six five-bit registers per word (register i -> word i / 6, shift 5 * (i % 6)),
 *                      exactly what ObjectSerDeUtils.HYPER_LOG_LOG_SER_DE#deserialize rebuilds (ObjectSerDeUtils.java:733-767)
 *   group key types    DataSchema column types of the group-by columns from the segment's column metadata (GroupByOperator.java:74-97)
 *
 * NOT compiled in this repository (no JDK in the build image): written against the reference's API by reading, see INTEGRATION.md.
 */
package org.apache.pinot.gpu;

import com.clearspring.analytics.stream.cardinality.HyperLogLog;
import com.clearspring.analytics.stream.cardinality.RegisterSet;
import it.unimi.dsi.fastutil.doubles.DoubleOpenHashSet;
import it.unimi.dsi.fastutil.floats.FloatOpenHashSet;
import it.unimi.dsi.fastutil.ints.IntOpenHashSet;
import it.unimi.dsi.fastutil.longs.LongOpenHashSet;
import it.unimi.dsi.fastutil.objects.ObjectOpenHashSet;
import java.util.List;
import java.util.Set;
import org.apache.pinot.common.request.context.ExpressionContext;
import org.apache.pinot.common.utils.DataSchema;
import org.apache.pinot.core.query.aggregation.function.AggregationFunction;
import org.apache.pinot.segment.spi.IndexSegment;
import org.apache.pinot.segment.spi.index.reader.Dictionary;
import org.apache.pinot.spi.data.FieldSpec.DataType;
import org.apache.pinot.spi.utils.ByteArray;

public final class GpuResultObjects {
  private GpuResultObjects() {
  }

  /** One value Set per group (empty sets for groups without a value: cannot happen for a group that exists). */
  @SuppressWarnings({"rawtypes", "unchecked"})
  public static Object[] valueSets(long result, int aggregation, int numGroups, IndexSegment segment, AggregationFunction function) {
    String column = ((ExpressionContext) function.getInputExpressions().get(0)).getIdentifier();
    Dictionary dictionary = segment.getDataSource(column).getDictionary();
    DataType stored = dictionary.getValueType();
    int[] sizes = new int[numGroups];
    PinotGpu.resultSetSizes(result, aggregation, sizes);
    long total = 0;
    for (int s : sizes) {
      total += s;
    }
    if (total > Integer.MAX_VALUE - 8) {
      throw new UnsupportedOperationException("DISTINCTCOUNT state of " + total + " dictIds exceeds one Java array");
    }
    int[] dictIds = new int[(int) total];
    PinotGpu.resultSetDictIds(result, aggregation, dictIds);
    Object[] out = new Object[numGroups];
    int at = 0;
    for (int g = 0; g < numGroups; g++) {
      int n = sizes[g];
      Set set;
      switch (stored) {
        case INT: {
          IntOpenHashSet s = new IntOpenHashSet(n);
          for (int i = 0; i < n; i++) {
            s.add(dictionary.getIntValue(dictIds[at + i]));
          }
          set = s;
          break;
        }
        case LONG: {
          LongOpenHashSet s = new LongOpenHashSet(n);
          for (int i = 0; i < n; i++) {
            s.add(dictionary.getLongValue(dictIds[at + i]));
          }
          set = s;
          break;
        }
        case FLOAT: {
          FloatOpenHashSet s = new FloatOpenHashSet(n);
          for (int i = 0; i < n; i++) {
            s.add(dictionary.getFloatValue(dictIds[at + i]));
          }
          set = s;
          break;
        }
        case DOUBLE: {
          DoubleOpenHashSet s = new DoubleOpenHashSet(n);
          for (int i = 0; i < n; i++) {
            s.add(dictionary.getDoubleValue(dictIds[at + i]));
          }
          set = s;
          break;
        }
        case STRING: {
          ObjectOpenHashSet<String> s = new ObjectOpenHashSet<>(n);
          for (int i = 0; i < n; i++) {
            s.add(dictionary.getStringValue(dictIds[at + i]));
          }
          set = s;
          break;
        }
        case BYTES: {
          ObjectOpenHashSet<ByteArray> s = new ObjectOpenHashSet<>(n);
          for (int i = 0; i < n; i++) {
            s.add(new ByteArray(dictionary.getBytesValue(dictIds[at + i])));
          }
          set = s;
          break;
        }
        default:
          throw new IllegalStateException("Illegal data type for DISTINCT_AGGREGATE aggregation function: " + stored);
      }
      out[g] = set;
      at += n;
    }
    return out;
  }

  /** DISTINCTCOUNT over a raw (no-dictionary) INT / LONG / FLOAT / DOUBLE column (pg_result_kind PG_RESULT_VALUE_SET): the library hands the
   *  groups' VALUES over — the typed open-hash sets BaseDistinctAggregateAggregationFunction.java:325-380 keeps for such a column. */
  @SuppressWarnings("rawtypes")
  public static Object[] rawValueSets(long result, int aggregation, int numGroups, IndexSegment segment, AggregationFunction function) {
    String column = ((ExpressionContext) function.getInputExpressions().get(0)).getIdentifier();
    DataType stored = segment.getDataSource(column).getDataSourceMetadata().getDataType().getStoredType();
    int[] sizes = new int[numGroups];
    PinotGpu.resultSetSizes(result, aggregation, sizes);
    long total = 0;
    for (int s : sizes) {
      total += s;
    }
    if (total > Integer.MAX_VALUE - 8) {
      throw new UnsupportedOperationException("DISTINCTCOUNT state of " + total + " values exceeds one Java array");
    }
    boolean floating = stored == DataType.FLOAT || stored == DataType.DOUBLE;
    long[] longs = floating ? null : new long[(int) total];
    double[] doubles = floating ? new double[(int) total] : null;
    if (floating) {
      PinotGpu.resultSetValuesDouble(result, aggregation, doubles);
    } else {
      PinotGpu.resultSetValuesLong(result, aggregation, longs);
    }
    Object[] out = new Object[numGroups];
    int at = 0;
    for (int g = 0; g < numGroups; g++) {
      int n = sizes[g];
      Set set;
      switch (stored) {
        case INT: {
          IntOpenHashSet s = new IntOpenHashSet(n);
          for (int i = 0; i < n; i++) {
            s.add((int) longs[at + i]);
          }
          set = s;
          break;
        }
        case LONG: {
          LongOpenHashSet s = new LongOpenHashSet(n);
          for (int i = 0; i < n; i++) {
            s.add(longs[at + i]);
          }
          set = s;
          break;
        }
        case FLOAT: {
          FloatOpenHashSet s = new FloatOpenHashSet(n);
          for (int i = 0; i < n; i++) {
            s.add((float) doubles[at + i]);   // widened exactly by the library
          }
          set = s;
          break;
        }
        case DOUBLE: {
          DoubleOpenHashSet s = new DoubleOpenHashSet(n);
          for (int i = 0; i < n; i++) {
            s.add(doubles[at + i]);
          }
          set = s;
          break;
        }
        default:
          throw new IllegalStateException("Illegal data type for a raw DISTINCT_AGGREGATE value set: " + stored);
      }
      out[g] = set;
      at += n;
    }
    return out;
  }

  /** PERCENTILE (pg_result_kind PG_RESULT_VALUE_COUNTS): per group the reference's DoubleArrayList of every matching value, expanded from the
   *  library's ascending (value, count) runs — merge is addAll and extractFinalResult sorts, so the order is free
   *  (PercentileAggregationFunction.java:139-171). */
  public static Object[] doubleLists(long result, int aggregation, int numGroups) {
    int[] sizes = new int[numGroups];
    PinotGpu.resultSetSizes(result, aggregation, sizes);
    long total = 0;
    for (int s : sizes) {
      total += s;
    }
    if (total > Integer.MAX_VALUE - 8) {
      throw new UnsupportedOperationException("PERCENTILE state of " + total + " runs exceeds one Java array");
    }
    double[] values = new double[(int) total];
    long[] counts = new long[(int) total];
    PinotGpu.resultSetValuesDouble(result, aggregation, values);
    PinotGpu.resultSetCounts(result, aggregation, counts);
    Object[] out = new Object[numGroups];
    int at = 0;
    for (int g = 0; g < numGroups; g++) {
      long n = 0;
      for (int i = 0; i < sizes[g]; i++) {
        n += counts[at + i];
      }
      if (n > Integer.MAX_VALUE - 8) {
        throw new UnsupportedOperationException("PERCENTILE list of " + n + " values exceeds one Java array");
      }
      double[] list = new double[(int) n];
      int k = 0;
      for (int i = 0; i < sizes[g]; i++) {
        java.util.Arrays.fill(list, k, k + (int) counts[at + i], values[at + i]);
        k += (int) counts[at + i];
      }
      out[g] = it.unimi.dsi.fastutil.doubles.DoubleArrayList.wrap(list);
      at += sizes[g];
    }
    return out;
  }

  /** VAR_POP / VAR_SAMP / STDDEV_POP / STDDEV_SAMP (pg_result_kind PG_RESULT_VARIANCE_TUPLE): per group the function's VarianceTuple from the
   *  library's three components — the count, the exact sum rounded once, the exact m2 rounded once.  Tuples of several segments merge with
   *  VarianceTuple#apply (VarianceAggregationFunction#merge), as the reference's own do. */
  public static Object[] varianceTuples(long result, int aggregation, int numGroups) {
    long[] count = new long[numGroups];
    double[] sum = new double[numGroups];
    double[] m2 = new double[numGroups];
    PinotGpu.resultLongs(result, aggregation, 0, count);
    PinotGpu.resultDoubles(result, aggregation, 0, sum);
    PinotGpu.resultDoubles(result, aggregation, 1, m2);
    Object[] out = new Object[numGroups];
    for (int g = 0; g < numGroups; g++) {
      out[g] = new org.apache.pinot.segment.local.customobject.VarianceTuple(count[g], sum[g], m2[g]);
    }
    return out;
  }

  /** MODE (pg_result_kind PG_RESULT_VALUE_COUNT_MAP): per group the function's map value -> count, typed by the column's stored type as
   *  ModeAggregationFunction types it — Int2LongOpenHashMap / Long2LongOpenHashMap / Float2LongOpenHashMap / Double2LongOpenHashMap; a group
   *  without a value gets the empty Int2LongOpenHashMap, whatever the column.  INT / LONG keys arrive exactly (resultSetValuesLong), FLOAT /
   *  DOUBLE keys as doubles (resultSetValuesDouble, a FLOAT widened exactly).  Maps of several segments merge by the per-key sum
   *  (ModeAggregationFunction#merge), as the reference's own do. */
  public static Object[] modeMaps(long result, int aggregation, int numGroups, IndexSegment segment, AggregationFunction function) {
    String column = ((ExpressionContext) function.getInputExpressions().get(0)).getIdentifier();
    DataType stored = segment.getDataSource(column).getDataSourceMetadata().getDataType().getStoredType();
    int[] sizes = new int[numGroups];
    PinotGpu.resultSetSizes(result, aggregation, sizes);
    long total = 0;
    for (int s : sizes) {
      total += s;
    }
    if (total > Integer.MAX_VALUE - 8) {
      throw new UnsupportedOperationException("MODE state of " + total + " entries exceeds one Java array");
    }
    boolean floating = stored == DataType.FLOAT || stored == DataType.DOUBLE;
    long[] longs = new long[floating ? 0 : (int) total];
    double[] doubles = new double[floating ? (int) total : 0];
    if (floating) {
      PinotGpu.resultSetValuesDouble(result, aggregation, doubles);
    } else {
      PinotGpu.resultSetValuesLong(result, aggregation, longs);
    }
    long[] counts = new long[(int) total];
    PinotGpu.resultSetCounts(result, aggregation, counts);
    Object[] out = new Object[numGroups];
    int at = 0;
    for (int g = 0; g < numGroups; g++) {
      int n = sizes[g];
      if (n == 0) {
        out[g] = new it.unimi.dsi.fastutil.ints.Int2LongOpenHashMap();
        continue;
      }
      switch (stored) {
        case INT: {
          it.unimi.dsi.fastutil.ints.Int2LongOpenHashMap m = new it.unimi.dsi.fastutil.ints.Int2LongOpenHashMap(n);
          for (int e = at; e < at + n; e++) {
            m.put((int) longs[e], counts[e]);
          }
          out[g] = m;
          break;
        }
        case LONG: {
          it.unimi.dsi.fastutil.longs.Long2LongOpenHashMap m = new it.unimi.dsi.fastutil.longs.Long2LongOpenHashMap(n);
          for (int e = at; e < at + n; e++) {
            m.put(longs[e], counts[e]);
          }
          out[g] = m;
          break;
        }
        case FLOAT: {
          it.unimi.dsi.fastutil.floats.Float2LongOpenHashMap m = new it.unimi.dsi.fastutil.floats.Float2LongOpenHashMap(n);
          for (int e = at; e < at + n; e++) {
            m.put((float) doubles[e], counts[e]);
          }
          out[g] = m;
          break;
        }
        default: {
          it.unimi.dsi.fastutil.doubles.Double2LongOpenHashMap m = new it.unimi.dsi.fastutil.doubles.Double2LongOpenHashMap(n);
          for (int e = at; e < at + n; e++) {
            m.put(doubles[e], counts[e]);
          }
          out[g] = m;
          break;
        }
      }
      at += n;
    }
    return out;
  }

  /** HISTOGRAM (pg_result_kind PG_RESULT_DOUBLE_ARRAY): per group the function's DoubleArrayList of numBins counts, as the library counted
   *  them.  Arrays of several segments merge with DoubleVectorOpUtils#vectorAdd (HistogramAggregationFunction#merge), as the reference's
   *  own do. */
  public static Object[] countArrays(long result, int aggregation, int numGroups) {
    int[] sizes = new int[numGroups];
    PinotGpu.resultSetSizes(result, aggregation, sizes);
    long total = 0;
    for (int s : sizes) {
      total += s;
    }
    if (total > Integer.MAX_VALUE - 8) {
      throw new UnsupportedOperationException("HISTOGRAM state of " + total + " bins exceeds one Java array");
    }
    double[] counts = new double[(int) total];
    PinotGpu.resultSetValuesDouble(result, aggregation, counts);
    Object[] out = new Object[numGroups];
    int at = 0;
    for (int g = 0; g < numGroups; g++) {
      out[g] = it.unimi.dsi.fastutil.doubles.DoubleArrayList.wrap(java.util.Arrays.copyOfRange(counts, at, at + sizes[g]));
      at += sizes[g];
    }
    return out;
  }

  /** SKEWNESS / KURTOSIS (pg_result_kind PG_RESULT_FOURTH_MOMENT): per group the function's PinotFourthMoment from the library's five
   *  components — n and the exact m1 .. m4, each rounded once.  The object's fields are inherited and protected: it is built from its own
   *  serialized form (PinotFourthMoment#serialize: long n, doubles m1 .. m4, big-endian).  Moments of several segments merge with
   *  PinotFourthMoment#combine (FourthMomentAggregationFunction#merge), as the reference's own do. */
  public static Object[] fourthMoments(long result, int aggregation, int numGroups) {
    long[] n = new long[numGroups];
    double[][] m = new double[4][numGroups];
    PinotGpu.resultLongs(result, aggregation, 0, n);
    for (int k = 0; k < 4; k++) {
      PinotGpu.resultDoubles(result, aggregation, k, m[k]);
    }
    Object[] out = new Object[numGroups];
    for (int g = 0; g < numGroups; g++) {
      java.nio.ByteBuffer bytes = java.nio.ByteBuffer.allocate(Long.BYTES + 4 * Double.BYTES);
      bytes.putLong(n[g]).putDouble(m[0][g]).putDouble(m[1][g]).putDouble(m[2][g]).putDouble(m[3][g]);
      out[g] = org.apache.pinot.segment.local.customobject.PinotFourthMoment.fromBytes(bytes.array());
    }
    return out;
  }

  /** COVAR_POP / COVAR_SAMP (pg_result_kind PG_RESULT_COVARIANCE_TUPLE): per group the function's CovarianceTuple from the library's four
   *  components — the exact sums of x, of y and of the rounded products, each rounded once, and the count.  Tuples of several segments merge
   *  with CovarianceTuple#apply (CovarianceAggregationFunction#merge), as the reference's own do. */
  public static Object[] covarianceTuples(long result, int aggregation, int numGroups) {
    double[] sumX = new double[numGroups];
    double[] sumY = new double[numGroups];
    double[] sumXY = new double[numGroups];
    long[] count = new long[numGroups];
    PinotGpu.resultDoubles(result, aggregation, 0, sumX);
    PinotGpu.resultDoubles(result, aggregation, 1, sumY);
    PinotGpu.resultDoubles(result, aggregation, 2, sumXY);
    PinotGpu.resultLongs(result, aggregation, 0, count);
    Object[] out = new Object[numGroups];
    for (int g = 0; g < numGroups; g++) {
      out[g] = new org.apache.pinot.segment.local.customobject.CovarianceTuple(sumX[g], sumY[g], sumXY[g], count[g]);
    }
    return out;
  }

  /** FIRSTWITHTIME / LASTWITHTIME (pg_result_kind PG_RESULT_VALUE_TIME_PAIR): per group the function's ValueLongPair of the declared type —
   *  the concrete subclass tells it — from the library's (value, time).  Pairs of several segments merge with the functions' own merge. */
  public static Object[] valueTimePairs(long result, int aggregation, int numGroups, AggregationFunction function) {
    long[] time = new long[numGroups];
    PinotGpu.resultLongs(result, aggregation, 0, time);
    Object[] out = new Object[numGroups];
    boolean isFloat = function instanceof org.apache.pinot.core.query.aggregation.function.FirstFloatValueWithTimeAggregationFunction
        || function instanceof org.apache.pinot.core.query.aggregation.function.LastFloatValueWithTimeAggregationFunction;
    boolean isDouble = function instanceof org.apache.pinot.core.query.aggregation.function.FirstDoubleValueWithTimeAggregationFunction
        || function instanceof org.apache.pinot.core.query.aggregation.function.LastDoubleValueWithTimeAggregationFunction;
    if (isFloat || isDouble) {
      double[] value = new double[numGroups];
      PinotGpu.resultDoubles(result, aggregation, 0, value);
      for (int g = 0; g < numGroups; g++) {
        out[g] = isFloat ? new org.apache.pinot.segment.local.customobject.FloatLongPair((float) value[g], time[g])   // widened exactly: the cast is exact
            : new org.apache.pinot.segment.local.customobject.DoubleLongPair(value[g], time[g]);
      }
      return out;
    }
    boolean isLong = function instanceof org.apache.pinot.core.query.aggregation.function.FirstLongValueWithTimeAggregationFunction
        || function instanceof org.apache.pinot.core.query.aggregation.function.LastLongValueWithTimeAggregationFunction;
    long[] value = new long[numGroups];
    PinotGpu.resultLongs(result, aggregation, 1, value);
    for (int g = 0; g < numGroups; g++) {
      out[g] = isLong ? new org.apache.pinot.segment.local.customobject.LongLongPair(value[g], time[g])
          : new org.apache.pinot.segment.local.customobject.IntLongPair((int) value[g], time[g]);
    }
    return out;
  }

  /** One HyperLogLog per group from its 2^log2m register bytes. */
  public static Object[] hyperLogLogs(long result, int aggregation, int numGroups, AggregationFunction function) {
    int log2m = ((org.apache.pinot.core.query.aggregation.function.DistinctCountHLLAggregationFunction) function).getLog2m();
    int m = 1 << log2m;
    long total = (long) numGroups * m;
    if (total > Integer.MAX_VALUE - 8) {
      throw new UnsupportedOperationException("HyperLogLog state of " + total + " registers exceeds one Java array");
    }
    byte[] registers = new byte[(int) total];
    PinotGpu.resultHllRegisters(result, aggregation, registers);
    Object[] out = new Object[numGroups];
    int words = (m + 5) / 6;   // RegisterSet.getSizeForCount: six five-bit registers per int
    for (int g = 0; g < numGroups; g++) {
      int[] bits = new int[words];
      int base = g * m;
      for (int i = 0; i < m; i++) {
        bits[i / 6] |= (registers[base + i] & 0x1F) << (5 * (i % 6));
      }
      out[g] = new HyperLogLog(log2m, new RegisterSet(m, bits));
    }
    return out;
  }

  /**
   * DataSchema column types of the group-by columns (GroupByOperator.java:74-97 takes them from the expressions' result metadata): the
   * column's type, DOUBLE for an arithmetic expression (the result metadata of the add / sub / mult / div transform functions), LONG for a
   * time-bucket transform (LONG_SV_NO_DICTIONARY_METADATA).
   */
  public static DataSchema.ColumnDataType[] keyTypes(IndexSegment segment, List<ExpressionContext> groupBy) {
    DataSchema.ColumnDataType[] types = new DataSchema.ColumnDataType[groupBy.size()];
    for (int i = 0; i < types.length; i++) {
      if (groupBy.get(i).getType() != ExpressionContext.Type.IDENTIFIER) {
        types[i] = NativeQuery.isTimeBucket(groupBy.get(i)) ? DataSchema.ColumnDataType.LONG : DataSchema.ColumnDataType.DOUBLE;
        continue;
      }
      DataType dataType = segment.getDataSource(groupBy.get(i).getIdentifier()).getDataSourceMetadata().getDataType();
      types[i] = DataSchema.ColumnDataType.fromDataTypeSV(dataType);
    }
    return types;
  }

  /**
   * The stored type's name behind a key: the column's, DOUBLE for an arithmetic expression (its values come back as DOUBLE value keys), LONG
   * for a time-bucket transform (LONG value keys).
   */
  public static String keyStoredType(IndexSegment segment, ExpressionContext key) {
    if (key.getType() != ExpressionContext.Type.IDENTIFIER) {
      return NativeQuery.isTimeBucket(key) ? "LONG" : "DOUBLE";
    }
    return segment.getDataSource(key.getIdentifier()).getDataSourceMetadata().getDataType().getStoredType().name();
  }
}
