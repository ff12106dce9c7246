/**
 * Selection operator of the accelerated path (pinot-core/.../operator/query/SelectionOnlyOperator.java, SelectionOrderByOperator.java,
 * EmptySelectionOperator.java): one pg_query_exec with PG_QUERY_FLAG_SELECTION per segment.  The rows come back as group keys over the
 * output columns in SelectionOperatorUtils#extractExpressions order (dictIds decoded through the segment's Dictionary, or the values of raw
 * columns) and fill a SelectionResultsBlock with the segment's ExecutionStatistics.  Under ORDER BY the rows are already sorted and the
 * block carries OrderByComparatorFactory's comparator, as SelectionOrderByOperator's does, so that the stock SelectionCombineOperator and the
 * broker reduce merge them with the blocks of segments the Java plan answered.
 */
package org.apache.pinot.gpu;

import java.nio.charset.StandardCharsets;
import java.util.ArrayList;
import java.util.Arrays;
import java.util.Collections;
import java.util.Comparator;
import java.util.List;
import java.util.function.Supplier;
import org.apache.pinot.common.request.context.ExpressionContext;
import org.apache.pinot.common.request.context.OrderByExpressionContext;
import org.apache.pinot.common.utils.DataSchema;
import org.apache.pinot.core.common.Operator;
import org.apache.pinot.core.operator.BaseOperator;
import org.apache.pinot.core.operator.ExecutionStatistics;
import org.apache.pinot.core.operator.blocks.results.BaseResultsBlock;
import org.apache.pinot.core.operator.blocks.results.SelectionResultsBlock;
import org.apache.pinot.core.query.request.context.QueryContext;
import org.apache.pinot.core.query.utils.OrderByComparatorFactory;
import org.apache.pinot.segment.spi.IndexSegment;
import org.apache.pinot.segment.spi.index.reader.Dictionary;

public class GpuSelectionOperator extends BaseOperator<BaseResultsBlock> {
  private static final String EXPLAIN_NAME = "GPU_SELECTION";

  private final IndexSegment _segment;
  private final QueryContext _queryContext;
  private final List<ExpressionContext> _expressions;   // extractExpressions: what NativeQuery.fromSelection put in the group-by slots
  private final long _segmentHandle;
  private final NativeQuery _nativeQuery;
  private final Supplier<Operator> _fallback;   // the default plan of this segment (a run-time PG_ERR_UNSUPPORTED: the sort tier's budget)
  private final long[] _stats = new long[5];
  private boolean _refused;

  public GpuSelectionOperator(IndexSegment segment, QueryContext queryContext, List<ExpressionContext> expressions, long segmentHandle,
      NativeQuery nativeQuery, Supplier<Operator> fallback) {
    _segment = segment;
    _queryContext = queryContext;
    _expressions = expressions;
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
      return blockOf(result);
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

  /** The rows as SelectionResultsBlock holds them: one Object[] per row over the output columns, typed by the columns' stored types. */
  private SelectionResultsBlock blockOf(long result) {
    int numColumns = _expressions.size();
    int numRows = PinotGpu.resultNumGroups(result);
    String[] names = new String[numColumns];
    for (int j = 0; j < numColumns; j++) {
      names[j] = _expressions.get(j).toString();
    }
    DataSchema dataSchema = new DataSchema(names, GpuResultObjects.keyTypes(_segment, _expressions));
    Object[][] values = new Object[numColumns][];
    for (int j = 0; j < numColumns; j++) {
      values[j] = columnValues(result, j, _expressions.get(j).getIdentifier(), numRows);
    }
    List<Object[]> rows = new ArrayList<>(numRows);
    for (int i = 0; i < numRows; i++) {
      Object[] row = new Object[numColumns];
      for (int j = 0; j < numColumns; j++) {
        row[j] = values[j][i];
      }
      rows.add(row);
    }
    List<OrderByExpressionContext> orderBy = _queryContext.getOrderByExpressions();
    if (orderBy == null || _queryContext.getLimit() == 0) {
      return new SelectionResultsBlock(dataSchema, rows, _queryContext);
    }
    // SelectionOrderByOperator's comparator: the ORDER BY expressions are the first output columns
    Comparator<Object[]> comparator = OrderByComparatorFactory.getComparator(orderBy, _queryContext.isNullHandlingEnabled());
    return new SelectionResultsBlock(dataSchema, rows, comparator, _queryContext);
  }

  /** One output column of the rows: dictIds through the segment's Dictionary, values of raw columns (BYTES as byte[], as the fetchers give). */
  private Object[] columnValues(long result, int j, String column, int numRows) {
    Object[] out = new Object[numRows];
    String storedType = _segment.getDataSource(column).getDataSourceMetadata().getDataType().getStoredType().name();
    int keyType = PinotGpu.resultGroupKeyType(result, j);
    if (keyType == PinotGpu.GROUP_KEY_LONG_VALUES) {
      long[] v = new long[numRows];
      PinotGpu.resultGroupValuesLong(result, j, v);
      for (int i = 0; i < numRows; i++) {
        out[i] = storedType.equals("INT") ? (Object) (int) v[i] : (Object) v[i];
      }
    } else if (keyType == PinotGpu.GROUP_KEY_DOUBLE_VALUES) {
      double[] v = new double[numRows];
      PinotGpu.resultGroupValuesDouble(result, j, v);
      for (int i = 0; i < numRows; i++) {
        out[i] = storedType.equals("FLOAT") ? (Object) (float) v[i] : (Object) v[i];
      }
    } else if (keyType == PinotGpu.GROUP_KEY_BYTES_VALUES) {
      long[] offsets = new long[numRows + 1];
      byte[] bytes = new byte[(int) PinotGpu.resultGroupValuesBytesSize(result, j)];
      PinotGpu.resultGroupValuesBytes(result, j, offsets, bytes);
      for (int i = 0; i < numRows; i++) {
        int from = (int) offsets[i], to = (int) offsets[i + 1];
        out[i] = storedType.equals("STRING") ? (Object) new String(bytes, from, to - from, StandardCharsets.UTF_8)
            : (Object) Arrays.copyOfRange(bytes, from, to);
      }
    } else {
      int[] dictIds = new int[numRows];
      PinotGpu.resultGroupDictIds(result, j, dictIds);
      Dictionary dictionary = _segment.getDataSource(column).getDictionary();
      for (int i = 0; i < numRows; i++) {
        switch (storedType) {
          case "INT": out[i] = dictionary.getIntValue(dictIds[i]); break;
          case "LONG": out[i] = dictionary.getLongValue(dictIds[i]); break;
          case "FLOAT": out[i] = dictionary.getFloatValue(dictIds[i]); break;
          case "DOUBLE": out[i] = dictionary.getDoubleValue(dictIds[i]); break;
          case "STRING": out[i] = dictionary.getStringValue(dictIds[i]); break;
          default: out[i] = dictionary.getBytesValue(dictIds[i]); break;
        }
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
