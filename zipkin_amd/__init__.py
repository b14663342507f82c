"""zipkin_amd — MI355X-native zipkin-aggregate dependency path.

The compute lives in libzkagg.so (HIP, gfx950) behind the C ABI of include/zkagg.h; this package
binds it (ctypes) and mirrors the reference's Aggregates store surface for the host side.
"""
from ._abi import ZkError, ZkLibraryError  # noqa: F401
from .columns import (ADJUSTED_TRACE_HEAD, ADJUSTED_TRACE_SPAN, BYTES_PER_RECORD, DeviceColumns, SpanColumns,  # noqa: F401
                      tracegen_host, tracegen_params)
from .context import DepsContext, LinkTable  # noqa: F401
from .realtime import LinkHistogram, LinkHistogramSnapshot  # noqa: F401
from .durations import TraceDurationIndex, TraceIdDuration, merge_top  # noqa: F401
from .nameindex import IndexedTraceId, TraceNameIndex, merge_trace_ids  # noqa: F401
from .annindex import AnnotationItems, DeviceAnnotationItems, TraceAnnotationIndex, get_trace_ids, trace_ids_intersect  # noqa: F401
from .retention import IndexRetention, SpanRetention  # noqa: F401
from .annotstore import ADJ_ANNOTATED, ADJ_OVERFLOW, ADJUSTED_HEAD, Annotation, AnnotationRows, DeviceAnnotationRows, Endpoint, TraceAnnotationStore  # noqa: F401
from .binannotstore import (BinaryAnnotation, BinaryAnnotationRows, DeviceBinaryAnnotationRows,  # noqa: F401
                            TraceBinaryAnnotationStore)
from .spanstore import (SUMMARY_HEAD, TRACE_HEAD, TRACE_SPAN, AnnotatedSpan, Span, SpanTimestamp, TimelineAnnotation,  # noqa: F401
                        Timespan, TimeSkewAdjuster, Trace, TraceCombo, TraceSpanStore, TraceSummary, TraceTimeline)
from .windows import WindowedAggregateJob, WindowPartition  # noqa: F401
from . import table  # noqa: F401

__all__ = [
    "ZkError",
    "ZkLibraryError",
    "SpanColumns",
    "DeviceColumns",
    "tracegen_host",
    "tracegen_params",
    "DepsContext",
    "LinkTable",
    "LinkHistogram",
    "LinkHistogramSnapshot",
    "WindowPartition",
    "WindowedAggregateJob",
    "TraceDurationIndex",
    "TraceIdDuration",
    "merge_top",
    "TraceNameIndex",
    "IndexedTraceId",
    "merge_trace_ids",
    "TraceAnnotationIndex",
    "AnnotationItems",
    "DeviceAnnotationItems",
    "get_trace_ids",
    "trace_ids_intersect",
    "IndexRetention",
    "SpanRetention",
    "TraceSpanStore",
    "Trace",
    "TraceSummary",
    "Span",
    "SpanTimestamp",
    "Timespan",
    "SUMMARY_HEAD",
    "TRACE_HEAD",
    "TRACE_SPAN",
    "TraceCombo",
    "TraceAnnotationStore",
    "TraceBinaryAnnotationStore",
    "BinaryAnnotationRows",
    "DeviceBinaryAnnotationRows",
    "BinaryAnnotation",
    "ADJUSTED_HEAD",
    "ADJUSTED_TRACE_HEAD",
    "ADJUSTED_TRACE_SPAN",
    "ADJ_ANNOTATED",
    "ADJ_OVERFLOW",
    "AnnotationRows",
    "DeviceAnnotationRows",
    "Annotation",
    "Endpoint",
    "AnnotatedSpan",
    "TimeSkewAdjuster",
    "TraceTimeline",
    "TimelineAnnotation",
    "BYTES_PER_RECORD",
]
