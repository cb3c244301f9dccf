"""Evaluators (reference: yolox/evaluators/__init__.py): the event-detection inference loop with COCO-style AP (EventEvaluator) or the
Prophesee protocol (PSEEEvaluator); VOC metric code is outside the hot path."""
from .event_evaluator import EventEvaluator
from .psee_evaluator import PSEEEvaluator

__all__ = ['EventEvaluator', 'PSEEEvaluator']
