/**
 * DistinctOperator of the accelerated path (pinot-core/.../operator/query/DistinctOperator.java, DictionaryBasedDistinctOperator.java): one
 * pg_query_exec with PG_QUERY_FLAG_DISTINCT per segment.  The tuples come back as group keys (dictIds decoded through the segment's
 * Dictionary, or the values of raw columns) and fill the reference's own tables — a typed single-column table (Int/Long/Float/Double/String/
 * BytesDistinctTable, what DistinctExecutor#getResult hands over for one column) or a MultiColumnDistinctTable — so that the stock
 * DistinctCombineOperator and the broker reduce merge them with the tables of segments the Java plan answered.  The library already kept at
 * most `limit` tuples (the top ones under ORDER BY): every one is added with addUnbounded.
 */
package org.apache.pinot.gpu;

import java.util.Collections;
import java.util.List;
import java.util.function.Supplier;
import org.apache.pinot.common.request.context.ExpressionContext;
import org.apache.pinot.common.request.context.OrderByExpressionContext;
import org.apache.pinot.common.utils.DataSchema;
import org.apache.pinot.core.common.Operator;
import org.apache.pinot.core.data.table.Record;
import org.apache.pinot.core.operator.BaseOperator;
import org.apache.pinot.core.operator.ExecutionStatistics;
import org.apache.pinot.core.operator.blocks.results.BaseResultsBlock;
import org.apache.pinot.core.operator.blocks.results.DistinctResultsBlock;
import org.apache.pinot.core.query.distinct.table.BytesDistinctTable;
import org.apache.pinot.core.query.distinct.table.DistinctTable;
import org.apache.pinot.core.query.distinct.table.DoubleDistinctTable;
import org.apache.pinot.core.query.distinct.table.FloatDistinctTable;
import org.apache.pinot.core.query.distinct.table.IntDistinctTable;
import org.apache.pinot.core.query.distinct.table.LongDistinctTable;
import org.apache.pinot.core.query.distinct.table.MultiColumnDistinctTable;
import org.apache.pinot.core.query.distinct.table.StringDistinctTable;
import org.apache.pinot.core.query.request.context.QueryContext;
import org.apache.pinot.segment.spi.IndexSegment;
import org.apache.pinot.segment.spi.index.reader.Dictionary;
import org.apache.pinot.spi.utils.ByteArray;

public class GpuDistinctOperator extends BaseOperator<BaseResultsBlock> {
  private static final String EXPLAIN_NAME = "GPU_DISTINCT";

  private final IndexSegment _segment;
  private final QueryContext _queryContext;
  private final long _segmentHandle;
  private final NativeQuery _nativeQuery;
  private final Supplier<Operator> _fallback;   // the default plan of this segment (a run-time PG_ERR_UNSUPPORTED)
  private final long[] _stats = new long[5];
  private boolean _refused;

  public GpuDistinctOperator(IndexSegment segment, QueryContext queryContext, long segmentHandle, NativeQuery nativeQuery,
      Supplier<Operator> fallback) {
    _segment = segment;
    _queryContext = queryContext;
    _segmentHandle = segmentHandle;
    _nativeQuery = nativeQuery;
    _fallback = fallback;
  }

  @Override
  protected BaseResultsBlock getNextBlock() {
    long result = execute();
    if (_refused) {
      return (BaseResultsBlock) _fallback.get().nextBlock();
    }
    try {
      return new DistinctResultsBlock(tableOf(result), _queryContext);
    } finally {
      PinotGpu.resultFree(result);
    }
  }

  private long execute() {
    long cancel = PinotGpu.cancelCreate();
    GpuCancellation.register(Thread.currentThread(), cancel);   // the query killer calls PinotGpu.cancelRequest(token) when it interrupts
    try {
      long result = PinotGpu.queryExec(_segmentHandle, _nativeQuery.address(), cancel);   // EarlyTerminationException when cancelled
      PinotGpu.resultStats(result, _stats);
      return result;
    } catch (UnsupportedOperationException e) {
      _refused = true;
      return 0;
    } finally {
      GpuCancellation.unregister(Thread.currentThread());
      PinotGpu.cancelDestroy(cancel);
      _nativeQuery.close();
    }
  }

  /** The result's tuples as the reference's distinct table of this query (DistinctExecutorFactory's DataSchema: expression names, SV types). */
  private DistinctTable tableOf(long result) {
    List<ExpressionContext> columns = _queryContext.getSelectExpressions();
    int numColumns = columns.size();
    int numRows = PinotGpu.resultNumGroups(result);
    String[] names = new String[numColumns];
    for (int j = 0; j < numColumns; j++) {
      names[j] = columns.get(j).toString();
    }
    DataSchema.ColumnDataType[] types = GpuResultObjects.keyTypes(_segment, columns);
    DataSchema dataSchema = new DataSchema(names, types);
    Object[][] values = new Object[numColumns][];
    for (int j = 0; j < numColumns; j++) {
      values[j] = columnValues(result, j, columns.get(j), numRows);
    }
    int limit = _queryContext.getLimit();
    boolean nullHandling = _queryContext.isNullHandlingEnabled();
    List<OrderByExpressionContext> orderBy = _queryContext.getOrderByExpressions();
    if (numColumns > 1) {
      MultiColumnDistinctTable table = new MultiColumnDistinctTable(dataSchema, limit, nullHandling, orderBy);
      for (int i = 0; i < numRows; i++) {
        Object[] row = new Object[numColumns];
        for (int j = 0; j < numColumns; j++) {
          row[j] = values[j][i];
        }
        table.addUnbounded(new Record(row));
      }
      return table;
    }
    OrderByExpressionContext order = orderBy == null ? null : orderBy.get(0);
    Object[] v = values[0];
    switch (types[0].getStoredType()) {
      case INT: {
        IntDistinctTable t = new IntDistinctTable(dataSchema, limit, nullHandling, order);
        for (Object o : v) {
          t.addUnbounded((Integer) o);
        }
        return t;
      }
      case LONG: {
        LongDistinctTable t = new LongDistinctTable(dataSchema, limit, nullHandling, order);
        for (Object o : v) {
          t.addUnbounded((Long) o);
        }
        return t;
      }
      case FLOAT: {
        FloatDistinctTable t = new FloatDistinctTable(dataSchema, limit, nullHandling, order);
        for (Object o : v) {
          t.addUnbounded((Float) o);
        }
        return t;
      }
      case DOUBLE: {
        DoubleDistinctTable t = new DoubleDistinctTable(dataSchema, limit, nullHandling, order);
        for (Object o : v) {
          t.addUnbounded((Double) o);
        }
        return t;
      }
      case STRING: {
        StringDistinctTable t = new StringDistinctTable(dataSchema, limit, nullHandling, order);
        for (Object o : v) {
          t.addUnbounded((String) o);
        }
        return t;
      }
      default: {
        BytesDistinctTable t = new BytesDistinctTable(dataSchema, limit, nullHandling, order);
        for (Object o : v) {
          t.addUnbounded(o instanceof ByteArray ? (ByteArray) o : new ByteArray((byte[]) o));
        }
        return t;
      }
    }
  }

  /**
   * One column of the tuples: dictIds through the segment's Dictionary (getInternal: the stored type), values of raw columns and of
   * arithmetic expressions (DOUBLE values) and of time-bucket transforms (LONG values).
   */
  private Object[] columnValues(long result, int j, ExpressionContext column, int numRows) {
    Object[] out = new Object[numRows];
    String storedType = GpuResultObjects.keyStoredType(_segment, column);
    int keyType = PinotGpu.resultGroupKeyType(result, j);
    if (keyType == PinotGpu.GROUP_KEY_LONG_VALUES) {
      long[] values = new long[numRows];
      PinotGpu.resultGroupValuesLong(result, j, values);
      for (int i = 0; i < numRows; i++) {
        out[i] = storedType.equals("INT") ? (Object) (int) values[i] : (Object) values[i];
      }
    } else if (keyType == PinotGpu.GROUP_KEY_DOUBLE_VALUES) {
      double[] values = new double[numRows];
      PinotGpu.resultGroupValuesDouble(result, j, values);
      for (int i = 0; i < numRows; i++) {
        out[i] = storedType.equals("FLOAT") ? (Object) (float) values[i] : (Object) values[i];
      }
    } else if (keyType == PinotGpu.GROUP_KEY_BYTES_VALUES) {
      long[] offsets = new long[numRows + 1];
      byte[] bytes = new byte[(int) PinotGpu.resultGroupValuesBytesSize(result, j)];
      PinotGpu.resultGroupValuesBytes(result, j, offsets, bytes);
      for (int i = 0; i < numRows; i++) {
        int from = (int) offsets[i], to = (int) offsets[i + 1];
        out[i] = storedType.equals("STRING") ? (Object) new String(bytes, from, to - from, java.nio.charset.StandardCharsets.UTF_8)
            : (Object) new ByteArray(java.util.Arrays.copyOfRange(bytes, from, to));
      }
    } else {
      int[] dictIds = new int[numRows];
      PinotGpu.resultGroupDictIds(result, j, dictIds);
      Dictionary dictionary = _segment.getDataSource(column.getIdentifier()).getDictionary();
      for (int i = 0; i < numRows; i++) {
        out[i] = dictionary.getInternal(dictIds[i]);
      }
    }
    return out;
  }

  @Override
  public List<Operator> getChildOperators() {
    return Collections.emptyList();
  }

  @Override
  public String toExplainString() {
    return EXPLAIN_NAME;
  }

  @Override
  public IndexSegment getIndexSegment() {
    return _segment;
  }

  @Override
  public ExecutionStatistics getExecutionStatistics() {
    return new ExecutionStatistics(_stats[0], _stats[1], _stats[2], _stats[3]);
  }
}
