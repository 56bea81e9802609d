"""Mirror of coati.common: the standard-library helpers of util.py (batch_indexable, ...).  coati.common.s3 is not provided."""
