"""Training callbacks with the names of kgcnn/training (the Keras callback protocol of ``gcnn_keras_amd.model.loop``)."""
