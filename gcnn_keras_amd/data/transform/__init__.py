"""Data transforms that run where the data is (kgcnn/data/transform): the label scalers of ``transform.scaler``."""
